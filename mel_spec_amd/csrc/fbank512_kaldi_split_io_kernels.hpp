// fbank512_kaldi_split_io_kernels.hpp -- the Kaldi fbank's split output with the sample type (float, int16_t) and the row type (float, f16,
// bf16) as template parameters: melspec_fbank_compute_*_device_split_io / melspec_fbank_compute_host_split_io.
//   fbank512_clip_split_io_kernel: fbank512_clip_kernel (fbank512_kernels.hpp: a workgroup owns whole clips, each of its eight f64 waves a
//     contiguous eighth of the clip's units) in its split mode, with typed loads (fb_kaldi_input<T, In>) and stores (fb_phase3_store<NSLOTS,
//     Out>).  It never subtracts: the rows leave un-normalised, each f32 value rounded to the row type once by its store, and the clip's
//     column means -- of the f32 values, before that rounding -- go to q.d_means.  The means are the f32 kernel's bits: the same per-wave
//     sums of the values a wave stores, the same fold over the four frame positions, the same eight partials in LDS, the same fixed tree of
//     the wave that arrives last, the same division.  One pass: 2 bytes per sample in, 2 bytes per element out, 4 * n_mels bytes per clip.
//   No 16-byte pieces are left (they were the subtraction's), so a clip may start at any sample and a clip's rows at any element.
//   What the subtraction's wait did besides waiting stays: a wave waits for the means of the workgroup's previous clip before it writes
//   its partials of this one or arrives for it, which keeps the waves within two clips of each other -- the two parity slots of
//   ClipCmnShared depend on it (fbank512_clip_kernel has the argument; tests/test_fbank_tiny_clips.py and tests/test_fbank_split_io.py
//   run workgroups over many clips whose waves have empty shares).
// Instantiated in a translation unit of their own (fbank512_kaldi_split_io.hip): a new neighbour in a unit changes the schedule of the
// kernels that are already there.
#pragma once
#include "fbank512_kernels.hpp"
#include "io_types.hpp"

namespace melspec {

// the means of the clip of parity `par` that is `expect` turns in are published (bounded like ClipCmnSub::wait: a mean that is never
// published would be a bug; a wrong result is caught by the parity tests, a hung GPU is not recoverable)
template <int WAVES>
MS_DEV void clip_split_wait(ClipCmnShared<WAVES> *sh, int par, unsigned expect, int lane) {
    for (unsigned spin = 0; spin < (1u << 22); ++spin) {
        bool ok = false;
        if (lane == 0) ok = __hip_atomic_load(&sh->ready[par], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >= expect;
        if (__builtin_amdgcn_ballot_w64(ok) != 0) break;
        __builtin_amdgcn_s_sleep(2);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int NSLOTS, class Lens, class In, class Out, bool RAGGED>
__global__ __launch_bounds__(8 * 64, 1) void fbank512_clip_split_io_kernel(const FbankClipParams q) {
    using T = double;
    using L = FbankLayout<T>;
    constexpr int WAVES = 8, NT = WAVES * 64;
    const FbankFastParams &p = q.f;
    extern __shared__ __attribute__((aligned(16))) uint32_t ldsw[];
    const int tid = threadIdx.x;
    for (int i = tid; i < p.blob_words; i += NT) ldsw[i] = p.d_blob[i];
    auto *sh = reinterpret_cast<ClipCmnShared<WAVES> *>(ldsw + p.blob_words + WAVES * L::slice_elems() * 2);
    if (tid < 2) { sh->arrived[tid] = 0; sh->ready[tid] = 0; }
    if (tid == 2) { sh->published = 0; sh->claimed = 0; }
    __syncthreads();
    const T *tblob = reinterpret_cast<const T *>(ldsw);
    const float *mel = reinterpret_cast<const float *>(ldsw + p.mel_off_words);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    T *slice = reinterpret_cast<T *>(ldsw + p.blob_words) + wave * L::slice_elems();
    const int fl = lane / kFbLanes, j = lane - fl * kFbLanes;
    int st[NSLOTS];
    {
        const int *starts = reinterpret_cast<const int *>(mel + FbankBlob::kMelStart);
#pragma unroll
        for (int i = 0; i < NSLOTS; ++i) st[i] = starts[i * kFbLanes + j];
    }
    const bool use_log = p.use_log != 0;
    const T preemph = static_cast<T>(p.preemph);
    const int nm = p.n_mels;
    unsigned gen = 0;                      // clips this workgroup has finished
    // uniform batches: clips blockIdx.x, + gridDim.x, ... of one length; ragged: the next clip of the batch's longest-first order
    for (unsigned seq = 0;; ++seq) {
        uint32_t clip;
        uint64_t frames;
        const In *pcm;                     // the plan counts elements: the two pointers are read as the kernel's own types
        Out *out;
        if (RAGGED) {
            clip = clip_queue_get<WAVES>(sh, seq, lane, p.b);
            if (clip == 0xffffffffu) break;
            frames = scalar64(p.b.d_frames[clip]);         // never 0: clips without a frame are not in the order
            pcm = reinterpret_cast<const In *>(p.b.pcm) + scalar64(p.b.d_off[clip]);
            out = reinterpret_cast<Out *>(p.b.out) + scalar64(p.b.d_out_off[clip]);
        } else {
            clip = blockIdx.x + seq * gridDim.x;
            if (clip >= p.b.n_clips) break;
            frames = q.frames;
            pcm = reinterpret_cast<const In *>(p.b.pcm) + (uint64_t)clip * p.b.clip_stride;
            out = reinterpret_cast<Out *>(p.b.out) + (uint64_t)clip * p.b.out_stride;
        }
        const uint32_t units = static_cast<uint32_t>((frames + kFbFPW - 1) / kFbFPW);
        const uint32_t u0 = static_cast<uint32_t>((uint64_t)units * wave / WAVES), u1 = static_cast<uint32_t>((uint64_t)units * (wave + 1) / WAVES);
        const int par = gen & 1;
        const unsigned prev_turn = (gen + 1) / 2;      // == (gen - 1) / 2 + 1 for gen > 0
        float acc[NSLOTS];
#pragma unroll
        for (int i = 0; i < NSLOTS; ++i) acc[i] = 0.0f;
        for (uint32_t u = u0; u < u1; ++u) {
            const uint64_t f0 = (uint64_t)u * kFbFPW;
            const uint64_t left = frames - f0;
            const int nv = left < (uint64_t)kFbFPW ? (int)left : kFbFPW;
            const bool act = fl < nv;
            MS_PRIO(0);
            const In *frame = pcm + (f0 + (uint64_t)(act ? fl : 0)) * (uint64_t)p.shift;
            // the frame mean, DC removal, pre-emphasis and the Povey window from ONE set of loads (fb_kaldi_input)
            if (act) {
                cpx<T> x[16];
                fb_kaldi_input<T>(frame, j, preemph, f0 + fl == 0 && j == 0, tblob, x);
                fb_column_finish<T>(x, j, tblob, slice + fl * L::kXStride);
            }
            __builtin_amdgcn_wave_barrier();
            MS_PRIO(1);
            {
                cpx<T> own[16], part[8];
                fb_phase2_dft<T>(fl, j, act, slice, own);
#pragma unroll
                for (int i = 0; i < 8; ++i) part[i] = {partner16(own[8 + i].re), partner16(own[8 + i].im)};
                fb_phase2_split<T, true>(fl, j, act, tblob, own, part, slice);       // power spectra only, as in fbank512_clip_kernel
            }
            __builtin_amdgcn_wave_barrier();
            MS_PRIO(2);
            float rise[NSLOTS], fprev[NSLOTS], fnext[NSLOTS], vals[NSLOTS];
            fb_phase3_sums<T, NSLOTS, Lens>(fl, j, act, p.slots, mel, slice, st, rise, fprev);
#pragma unroll
            for (int i = 0; i < NSLOTS; ++i) { fnext[i] = wave_shift_down1(fprev[i]); vals[i] = 0.0f; }
            fb_phase3_store<NSLOTS>(fl, j, act, nm, p.floor_v, use_log, rise, fnext, out + f0 * (uint64_t)nm, vals);
            // the f32 values, before the row type's rounding
#pragma unroll
            for (int i = 0; i < NSLOTS; ++i) acc[i] += vals[i];
            __builtin_amdgcn_wave_barrier();
        }
        MS_PRIO(0);
        // back-pressure: the means of clip c - 1 are published after all eight arrivals of c - 1, each of which came after that wave's wait
        // for clip c - 2 -- so clip c - 2 is folded before any wave writes part[par] or arrives on arrived[par] for clip c.  Without the
        // wait a wave with an empty share runs two clips ahead and arrives on a count that clip c - 2 has not completed
        if (gen > 0) clip_split_wait<WAVES>(sh, par ^ 1, prev_turn, lane);
        // the wave's column sums: frame positions (0+1)+(2+3), then lanes of position 0 write them
#pragma unroll
        for (int i = 0; i < NSLOTS; ++i) {
            acc[i] += __shfl_xor(acc[i], 16);
            acc[i] += __shfl_xor(acc[i], 32);
        }
        if (fl == 0 && j < kFbOwn) {
#pragma unroll
            for (int i = 0; i < NSLOTS; ++i)
                if (j + kFbOwn * i < nm) sh->part[par][wave][j + kFbOwn * i] = acc[i];
        }
        __builtin_amdgcn_wave_barrier();
        unsigned old = 0;
        if (lane == 0) old = __hip_atomic_fetch_add(&sh->arrived[par], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        const unsigned turn = gen / 2 + 1;      // how many clips of this parity, this one included
        if (__builtin_amdgcn_ballot_w64(lane == 0 && old == turn * WAVES - 1) != 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const float fr = static_cast<float>(frames);
            for (int m = lane; m < nm; m += 64) {
                const float (*pp)[96] = sh->part[par];
                const float s = ((pp[0][m] + pp[1][m]) + (pp[2][m] + pp[3][m])) + ((pp[4][m] + pp[5][m]) + (pp[6][m] + pp[7][m]));
                q.d_means[(uint64_t)clip * nm + m] = f32_div_rn(s, fr);
            }
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) __hip_atomic_store(&sh->ready[par], turn, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        ++gen;
    }
}

// The side table: the kernel of io = pcm_dtype | out_dtype << 4 for a uniform or a ragged batch (fbank_split_io_slot,
// fbank_split_io_plan.hpp); nullptr: no such kernel.  Defined beside the instantiations (fbank512_kaldi_split_io.hip).
using FbankClipSplitIoKernel = void (*)(const FbankClipParams);
FbankClipSplitIoKernel kaldi_split_io_kernel(bool ragged, int io);

}  // namespace melspec
