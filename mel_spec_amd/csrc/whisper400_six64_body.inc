// whisper400_six64_body.inc -- the body of whisper400_six64_kernel, included once per kernel that shares it (whisper400_kernels.hpp; the
// *_io_* kernels of whisper400_io_kernels.hpp) with MS_SIX64_IN / MS_SIX64_OUT = its sample and row types.  Text, not a function, like
// whisper400_six_runs_body.inc: the existing kernel must compile to the instructions it has.
// MS_SIX64_RAW (whisper_centered_kernels.hpp alone): the raw rows and the clip maximum of the centred Whisper features, as in
// whisper400_six_runs_body.inc.
    constexpr int WAVES = kSix64Waves;
    if (p.gate != nullptr && *p.gate != p.gate_value) return;        // the batch was light: the f32 launch has finished it
    extern __shared__ __attribute__((aligned(16))) uint32_t ldsw[];
    const int tid = threadIdx.x;
    for (int i = tid; i < p.blob_words; i += WAVES * 64) ldsw[i] = p.d_blob[i];
    unsigned *wg_done = ldsw + p.blob_words + WAVES * Six64Layout::slice_doubles() * 2;
    if (tid < 2) wg_done[tid] = 0;
    __syncthreads();
    const double *tb = reinterpret_cast<const double *>(ldsw);
    // the shared phase-3 code addresses the mel tables as offsets from the base of the six-frame f32 blob
    const float *fblob = reinterpret_cast<const float *>(ldsw + p.mel_off_words) - SixBlob::kMelStart;

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    double *rows = reinterpret_cast<double *>(ldsw + p.blob_words) + wave * Six64Layout::slice_doubles();
    float *slice = reinterpret_cast<float *>(rows);
    const int fl = lane / kSixLanes, j = lane - fl * kSixLanes;
    const bool in = lane < kSixFrames * kSixLanes;
    const int rofs = Six64Layout::row_offset(j);
    const int n_mels = Lens::kStatic ? Lens::kMels : p.n_mels;
    const int *starts = reinterpret_cast<const int *>(fblob + SixBlob::kMelStart) + j;
    const bool stats = p.stat.acc != nullptr;
    unsigned flagged = 0;
#ifdef MS_SIX64_RAW
    int rmax = 0;
#endif

    ClipRunT<MS_SIX64_IN, MS_SIX64_OUT> cr;
    if (!cr.init(p.b, (uint64_t)xcd_logical_block() * WAVES + wave, (uint64_t)gridDim.x * WAVES)) {
        guard_wave_done(p.stat, wg_done, WAVES, lane, 0);
        return;
    }
    for (; cr.unit < cr.end; ++cr.unit) {
#ifdef MS_SIX64_RAW
        if (cr.unit >= cr.c_end) { six_raw_flush(wc_slots, wc_slot_map, cr.clip, lane, rmax); rmax = 0; }
#endif
        cr.enter(p.b);
        const uint64_t f0 = (cr.unit - cr.c_start) * kSixFrames;
        const uint64_t left = cr.c_frames - f0;
        const int nv = left < (uint64_t)kSixFrames ? (int)left : kSixFrames;
        const MS_SIX64_IN *src = cr.c_pcm + f0 * (uint64_t)p.hop;
        const bool act = in && fl < nv;
        MS_PRIO(0);
        // The tables never change, and with __restrict__ the compiler knows it: left alone it hoists the unit loop's ~50 sixteen-byte table
        // reads out of the loop (200 VGPRs of "loop invariants"), spills them in front of the loop and reloads them from scratch inside it.
        // An offset it cannot see through makes the reads belong to the iteration.
        int opaque0 = 0;
        asm volatile("" : "+s"(opaque0));
        const double *tbi = tb + opaque0;
#ifdef MS_SIX64_RAW
        six64_phases12<MS_SIX64_IN, true>(fl, j, act, rofs, p.hop, tbi, src, rows, slice);        // int16 samples: all loads in front of the first conversion (six64_phase1)
#else
        six64_phases12(fl, j, act, rofs, p.hop, tbi, src, rows, slice);
#endif
        __builtin_amdgcn_wave_barrier();
        MS_PRIO(2);
        float vals[NSLOTS];
        {
            int st[NSLOTS];
#pragma unroll
            for (int i = 0; i < NSLOTS; ++i) st[i] = starts[i * kSixLanes];       // lanes 60..63 read valid entries too
            float rise[NSLOTS], fprev[NSLOTS], fnext[NSLOTS];
            six_phase3_sums<NSLOTS, Lens>(fl, j, act, p.slots, fblob, slice, st, rise, fprev);
#pragma unroll
            for (int i = 0; i < NSLOTS; ++i) fnext[i] = wave_shift_down1(fprev[i]);
            six_phase3_finish<NSLOTS>(fl, j, act, n_mels, rise, fnext, slice, vals);
        }
        __builtin_amdgcn_wave_barrier();
        MS_SIX64_OUT *out_tile = cr.c_out + f0 * (uint64_t)n_mels;
#ifdef MS_SIX64_RAW
        const bool flag = false;
        six_raw_store<NSLOTS>(fl, j, act, n_mels, vals, out_tile, rmax);
#else
        const bool flag = six_phase4<NSLOTS, false, true>(fl, j, act, act, n_mels, slice, vals, out_tile, 0);
#endif
        __builtin_amdgcn_wave_barrier();
        if (stats) flagged += static_cast<unsigned>(__builtin_popcount(frame_mask<kSixLanes, kSixFrames>(__builtin_amdgcn_ballot_w64(flag))));
    }
#ifdef MS_SIX64_RAW
    six_raw_flush(wc_slots, wc_slot_map, cr.clip, lane, rmax);
#endif
    guard_wave_done(p.stat, wg_done, WAVES, lane, flagged);
