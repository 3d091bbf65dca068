// fbank512_wave_body.inc -- the body of fbank512_wave_kernel (fbank512_kernels.hpp), included once per kernel that has it: the kernel itself
// (MS_FB512_IN = MS_FB512_OUT = float), fbank512_nemo_io_kernel (fbank512_io_kernels.hpp: int16 samples in, f16 / bf16 rows out, NeMo
// flavour) and fbank512_kaldi_io_kernel (fbank512_kaldi_io_kernels.hpp: the same ends, Kaldi flavour).  The including kernel provides T, WAVES, FLAVOR, NSLOTS, Lens, RUNS and the parameter p.
// MS_FB512_STATS (fbank512_nemo_stats_kernel, fbank512_stats_kernels.hpp: NeMo flavour, parameter q around p): the per-block partials of the
// split output next to the rows; without the macro the text below is what it always was.
// MS_FB512_STATS_RAGGED (on top of MS_FB512_STATS: fbank512_nemo_stats_ragged_kernel, fbank512_stats_ragged_kernels.hpp): the batch is a ragged
// one whose clips' unit counts are each a multiple of WAVES, the partials lie at [round of the batch][mel] and a block's valid frames come
// from the clip's own count; without the macro the text below is what it always was.
// MS_FB512_CONTINUES (fbank512_stream_kernel, fbank512_stream_kernels.hpp: Kaldi flavour, parameter q around p): q.d_cont[clip] != 0 says
// that the clip continues a stream -- the sample in front of its first frame exists and is that frame's predecessor (src/fbank.rs:177-181);
// without the macro the text below is what it always was.
// MS_FB512_CLIP_ORG0 (fbank512_nemo_stream_kernel, fbank512_nemo_stream_kernels.hpp: NeMo flavour, parameter q around p): the window origin
// of a clip's first frame is the clip's own, q.d_org0[clip], instead of the batch's p.org0; without the macro the text below is what it
// always was.
// MS_FB512_FRESH_FL (fbank512_nemo_stats_io_kernel, fbank512_stats_io_kernels.hpp): phase 2b's three row addresses in the wave's slice
// (fb_phase2_split: p, p + r, p - r) are derived from the lane's frame once per unit instead of being held across the unit loop -- the
// twelve-wave 128-mel kernel with int16 samples in is one VGPR short; without the macro the text below is what it always was.
#ifdef MS_FB512_FRESH_FL
#define MS_FB512_PHASE2_FL fresh_lane_value(fl)
#else
#define MS_FB512_PHASE2_FL fl
#endif
    using L = FbankLayout<T>;
    extern __shared__ __attribute__((aligned(16))) uint32_t ldsw[];
    const int tid = threadIdx.x;
    for (int i = tid; i < p.blob_words; i += WAVES * 64) ldsw[i] = p.d_blob[i];
    // NeMo: the feature-major store gives every wave 16 bytes of each mel row per unit; the units are walked in workgroup-uniform
    // rounds and the waves that hold adjacent units are kept in step before their stores (RoundSync, as in the mel-major Whisper kernels)
    constexpr bool ROUNDS = FLAVOR == kFlavorNemo;
    // the f32 NeMo kernel stages its feature-major rows in LDS (StagedRows) instead of keeping pairs of waves in step
    constexpr bool STAGE = FLAVOR == kFlavorNemo && sizeof(T) == 4;
    unsigned *arrive = ldsw + p.blob_words + WAVES * L::slice_elems() * (sizeof(T) / 4);     // 16 words: RoundSync counters; [15]: StagedRows
    if (ROUNDS && tid < 16) arrive[tid] = 0;
    __syncthreads();
    const T *tblob = reinterpret_cast<const T *>(ldsw);
    const float *mel = reinterpret_cast<const float *>(ldsw + p.mel_off_words);

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    T *slice = reinterpret_cast<T *>(ldsw + p.blob_words) + wave * L::slice_elems();
    const int fl = lane / kFbLanes, j = lane - fl * kFbLanes;
    const bool in = lane < kFbFPW * kFbLanes;
    // first bin of this lane's interval per slot: held across the unit loop by the compile-time banks; the run-time-lens variants
    // re-read the ten words in front of phase 3 instead (they sit at the 256-VGPR limit: holding them spilled inside the loop)
    int st[NSLOTS];
    const int *starts = reinterpret_cast<const int *>(mel + FbankBlob::kMelStart);
    // (the twelve-wave f32 NeMo kernel has no registers to hold them either)
    constexpr bool HOLD_STARTS = Lens::kStatic && !(FLAVOR == kFlavorNemo && sizeof(T) == 4);
    if (HOLD_STARTS) {
#pragma unroll
        for (int i = 0; i < NSLOTS; ++i) st[i] = in ? starts[i * kFbLanes + j] : 0;
    }
    const bool use_power = p.use_power != 0, use_log = p.use_log != 0;
    const T preemph = static_cast<T>(p.preemph);

    static_assert(!(RUNS && FLAVOR == kFlavorNemo), "the feature-major store wants adjacent units in adjacent waves");
    ClipRunT<MS_FB512_IN, MS_FB512_OUT> cr;
    if (RUNS && !cr.init(p.b, (uint64_t)xcd_logical_block() * WAVES + wave, (uint64_t)gridDim.x * WAVES)) return;
    RoundSync<WAVES> rs((ROUNDS && !STAGE) ? p.b.sync_rounds : 0, wave, arrive);
    StagedRows<STAGE ? WAVES : 4, MS_FB512_OUT> staged(arrive + 16, arrive + 15, p.n_mels);
#ifdef MS_FB512_STATS
    static_assert(FLAVOR == kFlavorNemo && !RUNS, "the partials are the NeMo flavour's");
    // f32: the block of the round that is drained next (this wave's previous round); f64: the waves' unit partials where the f32 kernel has
    // its images, counters arrive[8], [9]
    using SStats = StagedStats<STAGE ? WAVES : 4>;
    // the round's block of the batch, clip * blocks_per_clip + block = first / WAVES (the plan keeps it in 32 bits): counted, not divided
    uint32_t sblock = xcd_logical_block();
#ifdef MS_FB512_STATS_RAGGED
    // the partials of the round before this one: that round's block is its index among the batch's rounds, and its valid frames are what
    // the wave noted when it was in that round (another clip's, as often as not) -- one scalar, the kernel has no VGPR left
    int sn_prev = 0;
    auto sreduce = [&](unsigned r, int t) __attribute__((always_inline)) {
        SStats::reduce(staged, r, t, q.d_part + (uint64_t)(sblock - gridDim.x) * (uint64_t)p.n_mels, sn_prev);
    };
#else
    // the partials of the round before this one (its image has just been drained)
    auto sreduce = [&](unsigned r, int t) __attribute__((always_inline)) {
        const uint32_t sprev = sblock - gridDim.x, blk = sprev % q.blocks_per_clip;
        const uint64_t bf0 = (uint64_t)blk * (WAVES * kFbFPW), vf = p.b.frames_per_clip;
        const int n = vf > bf0 ? (vf - bf0 < (uint64_t)(WAVES * kFbFPW) ? (int)(vf - bf0) : WAVES * kFbFPW) : 0;
        SStats::reduce(staged, r, t, q.d_part + (uint64_t)sprev * (uint64_t)p.n_mels, n);
    };
#endif
    RoundStats<WAVES> rstats(arrive + 16, arrive + 8, p.n_mels);
#endif
    // batches planned on the device (plan_ragged_device_kernel) keep the real unit count in d_n_units; n_units is the host's bound
    const uint64_t n_units = RUNS ? 0 : scalar64(batch_n_units(p.b));
    // (STAGE with a contiguous range of units per workgroup instead of rounds dealt over the grid -- consecutive rounds extending the same
    // mel rows, no division per unit -- was measured: +1.4 %, profiles/r05_f32_512.txt)
    for (uint64_t first = (uint64_t)xcd_logical_block() * WAVES + (ROUNDS ? 0 : wave);; first += (uint64_t)gridDim.x * WAVES) {
        const uint64_t unit = ROUNDS ? first + rs.slot : first;
        if (RUNS) {
            if (cr.unit >= cr.end) break;
            cr.enter(p.b);
        } else if (first >= n_units) {
            break;
        }
        const bool have = !ROUNDS || unit < n_units;       // a wave without a unit idles through the round
        UnitLocT<MS_FB512_IN, MS_FB512_OUT> loc = RUNS ? cr.loc() : locate_unit<MS_FB512_IN, MS_FB512_OUT>(p.b, have ? unit : first);
        if (STAGE) loc = scalar_loc(loc);          // this kernel has no VGPRs for them
        const uint64_t f0 = loc.unit * kFbFPW;
        // valid frames of the clip (NeMo ragged: loc.frames is the padded width there)
        const uint64_t vframes = (FLAVOR == kFlavorNemo && p.d_valid) ? p.d_valid[loc.clip] : loc.frames;
        const uint64_t left = (have && f0 < vframes) ? vframes - f0 : 0;
        const int nv = left < (uint64_t)kFbFPW ? (int)left : kFbFPW;
        const bool act = in && fl < nv;
        MS_PRIO(0);
        if constexpr (FLAVOR == kFlavorKaldi) {
            const MS_FB512_IN *frame = loc.pcm + (f0 + (uint64_t)(act ? fl : 0)) * (uint64_t)p.shift;
            // the frame mean (src/fbank.rs:165-166: the frame's sixteen lanes, a fixed tree over DPP), DC removal, pre-emphasis and the Povey window
            // from ONE set of loads (fb_kaldi_input)
            if (act) {
                cpx<T> x[16];
#ifdef MS_FB512_CONTINUES
                fb_kaldi_input<T>(frame, j, preemph, f0 + fl == 0 && !q.d_cont[loc.clip] && j == 0, tblob, x);
#else
                fb_kaldi_input<T>(frame, j, preemph, f0 + fl == 0 && j == 0, tblob, x);
#endif
                fb_column_finish<T>(x, j, tblob, slice + fl * L::kXStride);
            }
        } else if constexpr (FLAVOR == kFlavorWhisper) {
            w512_phase1<T>(fl, j, act, loc.pcm + (f0 + (uint64_t)(act ? fl : 0)) * (uint64_t)p.shift, tblob, slice);
        } else {
            const long long clip_len = p.d_len ? (long long)p.d_len[loc.clip] : p.clip_len;
#ifdef MS_FB512_CLIP_ORG0
            const long long org = (long long)(f0 + (uint64_t)fl) * p.shift + q.d_org0[loc.clip];
#else
            const long long org = (long long)(f0 + (uint64_t)fl) * p.shift + p.org0;
#endif
            const bool inside = org >= 1 && org + 400 <= clip_len;
            const bool all_inside = __builtin_amdgcn_ballot_w64(act && !inside) == 0;
            nemo_phase1<T>(fl, j, act, all_inside, loc.pcm, org, clip_len, static_cast<float>(p.preemph), tblob, slice);
        }
        __builtin_amdgcn_wave_barrier();
        MS_PRIO(1);
        {
            cpx<T> own[16], part[8];
            fb_phase2_dft<T, STAGE>(fl, j, act, slice, own);
#pragma unroll
            for (int i = 0; i < 8; ++i) part[i] = {partner16(own[8 + i].re), partner16(own[8 + i].im)};
            if (FLAVOR == kFlavorWhisper) fb_phase2_split<T, true, sizeof(T) == 8>(fl, j, act, tblob, own, part, slice);      // f32: the amplitude form (fbank_tables.hpp)
            // NeMo: power spectra always (src/mel.rs:356-357) -- the magnitude form stays out of its unit loop (742 -> ~400 instructions in phase 2)
            else if (FLAVOR == kFlavorNemo || use_power) fb_phase2_split<T, true>(MS_FB512_PHASE2_FL, j, act, tblob, own, part, slice);
            else fb_phase2_split<T, false>(fl, j, act, tblob, own, part, slice);
        }
        __builtin_amdgcn_wave_barrier();
        MS_PRIO(2);
        float rise[NSLOTS], fprev[NSLOTS], fnext[NSLOTS];
        if (!HOLD_STARTS) {
            const int *mine = starts + (STAGE ? fresh_lane_value(j) : j);
#pragma unroll
            for (int i = 0; i < NSLOTS; ++i) st[i] = in ? mine[i * kFbLanes] : 0;
        }
        fb_phase3_sums<T, NSLOTS, Lens>(fl, j, act, p.slots, mel, slice, st, rise, fprev);
#pragma unroll
        for (int i = 0; i < NSLOTS; ++i) fnext[i] = wave_shift_down1(fprev[i]);
        if constexpr (FLAVOR == kFlavorKaldi) {
            fb_phase3_store<NSLOTS>(fl, j, act, p.n_mels, p.floor_v, use_log, rise, fnext, loc.out + f0 * (uint64_t)p.n_mels);
        } else if constexpr (FLAVOR == kFlavorWhisper) {
            float vals[NSLOTS];
            float *slice_f = reinterpret_cast<float *>(slice);
            w512_phase3_log<NSLOTS>(fl, j, act, p.n_mels, rise, fnext, slice_f, vals);
            __builtin_amdgcn_wave_barrier();
            // columns this unit stores: the clip's frames plus, for padded layouts, zero columns up to out_width
            const uint64_t width = p.b.d_unit_prefix == nullptr ? p.b.out_width : loc.frames;
            const uint64_t wleft = width - f0;
            const int ns = wleft < (uint64_t)kFbFPW ? (int)wleft : kFbFPW;
            if (p.b.mel_major)
                w512_phase4<NSLOTS>(fl, j, in && fl < ns, act, p.n_mels, slice_f, vals, loc.out + f0, (long long)width);
            else
                w512_phase4<NSLOTS>(fl, j, in && fl < ns, act, p.n_mels, slice_f, vals, loc.out + f0 * (uint64_t)p.n_mels, 0);
        } else {
            const uint64_t row_w = p.b.d_unit_prefix == nullptr ? p.b.out_width : loc.frames;
#ifdef MS_FB512_STATS
            const uint64_t wleft = (have && f0 < row_w) ? row_w - f0 : 0;      // the clip's units are rounded up to whole rounds: some lie past the row
            // the round's block (computed where it is used, by the one wave that uses it): WAVES units from unit blk * WAVES of the clip on,
            // nb valid frames, its partials at pdst
#ifdef MS_FB512_STATS_RAGGED
            // (every clip in front of this one has whole rounds: unit_prefix[clip] / WAVES + blk = first / WAVES, which sblock counts)
#define MS_FB512_STATS_BLOCK_INDEX (uint64_t)sblock
#else
#define MS_FB512_STATS_BLOCK_INDEX ((uint64_t)loc.clip * q.blocks_per_clip + blk)
#endif
#define MS_FB512_STATS_BLOCK                                                                                                             \
            const uint64_t blk = loc.unit / WAVES, bf0 = blk * (WAVES * kFbFPW);                                                         \
            const int nb = vframes > bf0 ? (vframes - bf0 < (uint64_t)(WAVES * kFbFPW) ? (int)(vframes - bf0) : WAVES * kFbFPW) : 0;     \
            float2 *const pdst = q.d_part + MS_FB512_STATS_BLOCK_INDEX * (uint64_t)p.n_mels;
#else
            const uint64_t wleft = have ? row_w - f0 : 0;
#endif
            const int ns = wleft < (uint64_t)kFbFPW ? (int)wleft : kFbFPW;
            if (STAGE) {
                float vals[NSLOTS];
#pragma unroll
                for (int i = 0; i < NSLOTS; ++i) vals[i] = act ? fast_ln((rise[i] + fnext[i]) + p.floor_v) : 0.0f;
#ifdef MS_FB512_STATS
                // the unit goes into its image first and the previous round is drained behind it, when the unit's values are out of the
                // registers (the reduction of the drained block needs them); the count is raised last: a wave that sees every wave's count for
                // round r knows that each has drained round r - 1, as it does without the partials
                if (staged.round > 0) staged.wait_staged(staged.round, lane);
                staged.template stage<NSLOTS>(wave, lane, vals, loc.out + f0, (long long)row_w, ns);
                if (staged.round > 0) {
                    int dtid = tid;
                    asm volatile("" : "+v"(dtid));          // see StagedRows::drain
                    staged.drain(staged.round - 1, dtid);
                    sreduce(staged.round - 1, dtid);
                }
#ifdef MS_FB512_STATS_RAGGED
                {
                    // this round's block for the next iteration: the round's first unit is this wave's less its slot
                    const uint64_t bf0 = (loc.unit - (uint64_t)rs.slot) * kFbFPW;
                    sn_prev = __builtin_amdgcn_readfirstlane(vframes > bf0 ? (vframes - bf0 < (uint64_t)(WAVES * kFbFPW) ? (int)(vframes - bf0) : WAVES * kFbFPW) : 0);
                }
#endif
                staged.publish(lane);
#else
                if (staged.round > 0) {
                    int dtid = tid;
                    asm volatile("" : "+v"(dtid));          // see StagedRows::drain
                    staged.wait_staged(staged.round, lane);
                    staged.drain(staged.round - 1, dtid);
                }
                staged.template put<NSLOTS>(wave, lane, vals, loc.out + f0, (long long)row_w, ns);
#endif
            } else {
                rs.template before_stores<2>(lane);
#ifndef MS_FB512_STATS
                nemo_phase3_store<NSLOTS>(fl, j, in && fl < ns, act, p.n_mels, p.floor_v, rise, fnext, loc.out + f0, (long long)row_w);
#else
                {
                    // nemo_phase3_store's values, computed ONCE for the rows and the partials: a second use of rise[i] keeps the compiler from
                    // contracting a one-bin interval's product into this sum the way the raw kernel's only use lets it, and the rows of the
                    // 128-mel bank (three such slots) then differ from the raw call's in the last place
                    float vals[NSLOTS];
#pragma unroll
                    for (int i = 0; i < NSLOTS; ++i) vals[i] = act ? fast_ln((rise[i] + fnext[i]) + p.floor_v) : 0.0f;
                    nemo_store_vals<NSLOTS>(fl, j, in && fl < ns, p.n_mels, vals, loc.out + f0, (long long)row_w);
                    // the unit's partial per mel row {c, squares around c} of its valid frames' values; c = the first frame's value + the mean
                    // distance from it (fbank512_stats_kernels.hpp says why)
                    rstats.wait_free(lane);
                    const float inv_nv = nv == 4 ? 0.25f : nv == 3 ? 0.333333343f : nv == 2 ? 0.5f : 1.0f;
                    float2 *mine = rstats.part + wave * p.n_mels + j;
#pragma unroll
                    for (int i = 0; i < NSLOTS; ++i) {
                        const float v = vals[i];
                        const float first = stats_sum_frames(lane < kFbLanes ? v : 0.0f);
                        const float d = act ? v - first : 0.0f;
                        const float shift = f32_mul_rn(stats_sum_frames(d), inv_nv);
                        const float e = act ? d - shift : 0.0f;
                        const float sq = stats_sum_frames(f32_mul_rn(e, e));
                        if (lane < kFbOwn && j + kFbOwn * i < p.n_mels) mine[kFbOwn * i] = make_float2(first + shift, sq);
                    }
                    MS_FB512_STATS_BLOCK
                    rstats.arrive(lane, pdst, nb);
                }
#endif
            }
        }
#ifdef MS_FB512_STATS
#undef MS_FB512_STATS_BLOCK
#undef MS_FB512_STATS_BLOCK_INDEX
#endif
        __builtin_amdgcn_wave_barrier();
        if (ROUNDS) rs.after_round();
        if (RUNS) ++cr.unit;
#ifdef MS_FB512_STATS
        sblock += gridDim.x;
#endif
    }
    if (STAGE && staged.round > 0) {
        staged.wait_staged(staged.round, lane);
        staged.drain(staged.round - 1, tid);
#ifdef MS_FB512_STATS
        sreduce(staged.round - 1, tid);
#endif
    }
#undef MS_FB512_PHASE2_FL
