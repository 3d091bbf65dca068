// fbank_split_io_plan.hpp -- the host side of the Kaldi fbank's split output (melspec_fbank_compute_ragged_device_split and the
// melspec_fbank_compute_*_split_io calls, fbank512.hip) that is arithmetic only: the dtype codes, the checks of the calls' arguments in
// their order, and the index of a kernel in the side table of fbank512_kaldi_split_io.hip.  The plans are the f32 calls' own (plan_uniform,
// plan_ragged by clip): they count elements.  Nothing from HIP in here: tests/cpp/fbank_split_io_host.cpp builds it on the host, with and
// without sanitizers.
#pragma once
#include "fused512_route.hpp"

namespace melspec {
namespace host {

// ---- the side table: [uniform, ragged][io_index of the (sample, row) combination] --------------------------------------------------------
constexpr int kFbankSplitIoCombos = 5;                                  // MS_IO_COMBOS: every pair but (F32, F32)
constexpr int kFbankSplitIoKernels = 2 * kFbankSplitIoCombos;
// < 0: io is (F32, F32) -- the f32 split calls' -- or not a combination at all
constexpr int fbank_split_io_slot(bool ragged, int io) { return io_index(io) < 0 ? -1 : (ragged ? kFbankSplitIoCombos : 0) + io_index(io); }
// the route whose launch shape (waves, LDS, grid rule) the kernel of a slot takes: the f32 clip kernel's of the same kind of batch
constexpr Batch512 fbank_split_io_batch(bool ragged) { return ragged ? Batch512::kClipRagged : Batch512::kClipUniform; }

// ---- the arguments ------------------------------------------------------------------------------------------------------------------------
constexpr bool fbank_split_io_pcm_known(int t) { return t == MELSPEC_PCM_F32 || t == MELSPEC_PCM_S16; }
constexpr bool fbank_split_io_out_known(int t) { return t == MELSPEC_OUT_F32 || t == MELSPEC_OUT_F16 || t == MELSPEC_OUT_BF16; }
constexpr size_t fbank_split_io_pcm_bytes(int t) { return t == MELSPEC_PCM_S16 ? 2 : 4; }
constexpr size_t fbank_split_io_out_bytes(int t) { return t == MELSPEC_OUT_F32 ? 4 : 2; }
inline bool fbank_split_io_misaligned(const void *pcm, int pcm_dtype, const void *rows, int out_dtype) {
    return (reinterpret_cast<uintptr_t>(pcm) & (fbank_split_io_pcm_bytes(pcm_dtype) - 1)) || (reinterpret_cast<uintptr_t>(rows) & (fbank_split_io_out_bytes(out_dtype) - 1));
}
// the object can run the 16-bit split: the fused path on eight f64 waves with the compile-time 80-bin Kaldi bank, CMN on power spectra
constexpr bool fbank_split_io_ok(const Fused512Shape &s, int nm) { return kaldi_io_ok(s) && clip_shape_ok(s, nm); }

// kFbankSplitZero: nothing to compute, but the clips' mean slots (where d_means is given) are to be zeroed -- no clip has a frame
enum FbankSplitVerdict { kFbankSplitGo = 0, kFbankSplitDone = 1, kFbankSplitZero = 2, kFbankSplitFail = 3 };
struct FbankSplitArgs {
    FbankSplitVerdict verdict;
    int status;
    const char *msg;        // kFbankSplitFail with nullptr: the caller words the error (the unsupported object: it names the geometry)
};
constexpr const char *kFbankSplitCmnOff = "the split output is the CMN's two halves: FbankConfig::apply_cmn is off";

// The object and the dtype codes: in front of everything else.  kFbankSplitGo: io = pcm_dtype | out_dtype << 4 (0: (F32, F32), which the
// caller hands to the f32 split call as it is).
inline FbankSplitArgs fbank_split_io_codes(bool have_fb, int pcm_dtype, int out_dtype, int &io) {
    io = 0;
    if (!have_fb) return {kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "fbank is NULL"};
    if (!fbank_split_io_pcm_known(pcm_dtype)) return {kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "pcm_dtype must be MELSPEC_PCM_F32 or MELSPEC_PCM_S16"};
    if (!fbank_split_io_out_known(out_dtype)) return {kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "out_dtype must be MELSPEC_OUT_F32, MELSPEC_OUT_F16 or MELSPEC_OUT_BF16"};
    io = pcm_dtype | out_dtype << 4;
    return {kFbankSplitGo, MELSPEC_OK, nullptr};
}
// Behind the codes, in this order: apply_cmn, the object's support, no clips, (ragged) the tables, no frame at all, the device pointers,
// d_means, the alignment of the two typed pointers.  io = 0: the f32 ragged split, which every object supports (`supported` true) and
// whose pointers are floats.  ragged false: h_offsets / h_lengths are not looked at.  total_frames: of the whole batch (the caller counts
// them only when the tables are there).
inline FbankSplitArgs fbank_split_args(bool apply_cmn, bool supported, bool ragged, uint32_t n_clips, const void *h_offsets, const void *h_lengths, uint64_t total_frames,
                                       const void *pcm, const void *rows, const void *means, int io) {
    if (!apply_cmn) return {kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, kFbankSplitCmnOff};
    if (!supported) return {kFbankSplitFail, MELSPEC_ERR_UNSUPPORTED, nullptr};
    if (n_clips == 0) return {kFbankSplitDone, MELSPEC_OK, nullptr};
    if (ragged && (!h_offsets || !h_lengths)) return {kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "offset/length array is NULL"};
    if (total_frames == 0) return {means ? kFbankSplitZero : kFbankSplitDone, MELSPEC_OK, nullptr};
    if (!pcm || !rows) return {kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "device pointer is NULL"};
    if (!means) return {kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "d_means is NULL"};
    if (fbank_split_io_misaligned(pcm, io & 15, rows, io >> 4)) return {kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type"};
    return {kFbankSplitGo, MELSPEC_OK, nullptr};
}

}  // namespace host
}  // namespace melspec
