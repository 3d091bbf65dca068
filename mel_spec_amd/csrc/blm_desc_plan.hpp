// blm_desc_plan.hpp -- the arithmetic of melspec_blm_compute_ragged_device_desc (fbank512.hip): a ragged batch of the NeMo / Parakeet
// frontend whose clip table lives in device memory.  What one clip needs -- valid frames for center 0 / 1, the pad_to rounding of the row
// width, units of four frames, the rejection of a clip longer than the caller's bound -- is here once, for the planner kernel
// (blm_plan_ragged_device_kernel, aux_kernels.hpp) and for the host; so are the layout of the plan buffer, the bounds the launch is
// sized from, the shape of the ragged normaliser, and a serial planner that fills the same tables from host arrays.  Nothing from HIP in
// here: tests/cpp/blm_desc_plan_host.cpp builds it on the host, with and without sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MS_BLM_HD __host__ __device__ inline
#else
#define MS_BLM_HD inline
#endif

namespace melspec {
namespace host {

constexpr uint32_t kBlmDescFramesPerUnit = 4;        // kFbFPW
constexpr uint32_t kBlmDescUnitBlock = 16;           // kUnitBlock
constexpr uint32_t kBlmDescNormThreads = 256;        // kBlmNormThreads

// what the planner reads of the context
struct BlmDescGeom {
    uint32_t n_fft, hop, pad_to;
    uint32_t center;          // 0 / 1
    uint32_t n_mels;
};

// valid frames of a clip of n samples (src/mel.rs:326-332,387-395) and the row width (pad_len, src/mel.rs:751-756)
MS_BLM_HD uint64_t blm_desc_valid_frames(const BlmDescGeom &g, uint64_t n) {
    if (n == 0) return 0;
    if (g.center) return n / g.hop + 1;
    if (n < g.n_fft) return 0;
    return (n - g.n_fft) / g.hop + 1;
}
MS_BLM_HD uint64_t blm_desc_padded(const BlmDescGeom &g, uint64_t frames) {
    return g.pad_to == 0 ? frames : (frames + g.pad_to - 1) / g.pad_to * g.pad_to;
}

// One clip of the device table.  Rule (A): a clip longer than max_clip_samples is rejected and planned as a clip of length 0 -- no
// rows, no units, no space in a packed output, and nothing of it is ever read.
struct BlmDescClip {
    uint64_t len;         // 0 when rejected
    uint64_t valid;       // valid frames
    uint64_t cols;        // row width, the plan's `frames`
    uint64_t units;       // ceil(cols / 4)
    bool rejected;
};
MS_BLM_HD BlmDescClip blm_desc_clip(const BlmDescGeom &g, uint64_t len, uint64_t max_clip_samples) {
    BlmDescClip c;
    c.rejected = len > max_clip_samples;
    c.len = c.rejected ? 0 : len;
    c.valid = blm_desc_valid_frames(g, c.len);
    c.cols = blm_desc_padded(g, c.valid);
    c.units = (c.cols + kBlmDescFramesPerUnit - 1) / kBlmDescFramesPerUnit;
    return c;
}

// ---- the ragged normaliser's shape ---------------------------------------------------------------------------------------------------
// rows staged per workgroup (`per`, 0: a row does not fit), the row stride in LDS and the workgroups per CU, for a batch whose longest
// clip has `longest` valid frames: rows staged whole in LDS like the uniform pass, groups of rows from a counter
MS_BLM_HD void blm_norm_shape_ragged(uint64_t longest, size_t &stride, size_t &per, int &per_cu) {
    stride = (static_cast<size_t>(longest) + 3 + 31) & ~static_cast<size_t>(31);
    if ((stride / 4) % 2 == 0) stride += 4;
    const size_t fixed = (2 * 64 + kBlmDescNormThreads + 4 * 64 + 4) * sizeof(float);
    per = (static_cast<size_t>(38) * 1024 - fixed) / (stride * sizeof(float));
    per_cu = 4;
    if (per < 4) { per = (static_cast<size_t>(150) * 1024 - fixed) / (stride * sizeof(float)); per_cu = 1; }
    if (per > 64) per = 64;
}
// The threads that share a row's sum of squares in the pass melspec_blm_compute_ragged_device launches for a batch whose longest clip has
// `longest` valid frames: 256 / per -- the ORDER of that sum, and so the bits of 1 / std.  0: that launch is the one-thread-per-row pass
// (a row does not fit LDS), whose sum is a left fold.  The _desc call sizes its launch from the caller's bound, which may be far above the
// batch's longest clip; the planner kernel, which sees the true lengths, notes this number and the _desc normalisers sum in its order,
// so that the bits do not depend on the bound.
MS_BLM_HD uint32_t blm_desc_norm_order(uint64_t longest) {
    size_t stride, per;
    int per_cu;
    blm_norm_shape_ragged(longest, stride, per, per_cu);
    if (per < 1 || longest >= (1ull << 31)) return 0;
    return kBlmDescNormThreads / static_cast<uint32_t>(per);
}

// The _desc normaliser's launch for a bound of `bound_valid` valid frames on the longest clip: blm_norm_shape_ragged, except that a row
// never has fewer threads than blm_desc_norm_order of any shorter clip asks for.  `per` is not monotonic: it falls to 4 as the clips
// grow, jumps up where the shape moves from four 38 KB workgroups per CU to one of 150 KB, and falls again.  Below the jump the bound's
// own shape has the fewest rows of all shorter clips; past it at most four rows are staged (64 threads per row, the most a shorter clip
// below the jump can ask for), and past-the-jump clips shorter than the bound ask for no more than the bound's own shape.
MS_BLM_HD void blm_desc_norm_launch(uint64_t bound_valid, size_t &stride, size_t &per, int &per_cu) {
    blm_norm_shape_ragged(bound_valid, stride, per, per_cu);
    if (per_cu == 1 && per > 4) per = 4;
}

// ---- what the host sizes from the caller's two bounds --------------------------------------------------------------------------------
// every clip with columns has at most cols / 4 + 1 units
MS_BLM_HD uint64_t blm_desc_max_units(uint64_t max_total_columns, uint32_t n_clips) { return max_total_columns / kBlmDescFramesPerUnit + n_clips; }
MS_BLM_HD uint64_t blm_desc_max_blocks(uint64_t max_units) { return max_units / kBlmDescUnitBlock + 2; }
// Do the bounds fit the plan's integer widths?  The normalisers keep a clip's valid frames and row width in 32 bits; the sums of the
// planner (columns, units, output floats = columns * n_mels) stay far inside 64 bits with a total below 2^40 columns.
MS_BLM_HD bool blm_desc_bounds_ok(const BlmDescGeom &g, uint64_t max_total_columns, uint64_t max_clip_samples) {
    if (max_clip_samples >= (1ull << 62) || max_total_columns >= (1ull << 40)) return false;
    return blm_desc_padded(g, blm_desc_valid_frames(g, max_clip_samples)) < (1ull << 31);
}

// ---- the plan buffer -----------------------------------------------------------------------------------------------------------------
// [off n][frames n][out_off n][prefix n + 1] u64 as plan_ragged lays them out (frames = the padded row width), then what the NeMo kernels
// read besides: [len n][valid n] u64, one word {the normaliser's group counter = 0, blm_desc_norm_order of the batch} (two u32), and the
// kUnitBlock block table (u32, max_blocks entries).
MS_BLM_HD size_t blm_desc_words64(uint32_t n_clips) { return static_cast<size_t>(n_clips) * 6 + 2; }
MS_BLM_HD size_t blm_desc_bytes(uint32_t n_clips, uint64_t max_blocks) {
    return blm_desc_words64(n_clips) * sizeof(uint64_t) + static_cast<size_t>(max_blocks) * sizeof(uint32_t) + 16;
}
struct BlmDescTables {
    uint64_t *off, *frames, *out_off, *prefix, *len, *valid;
    uint32_t *ctr, *order, *blk;
};
MS_BLM_HD BlmDescTables blm_desc_tables(uint64_t *buf, uint32_t n_clips) {
    BlmDescTables t;
    const size_t n = n_clips;
    t.off = buf; t.frames = buf + n; t.out_off = buf + 2 * n; t.prefix = buf + 3 * n;
    t.len = buf + 4 * n + 1; t.valid = buf + 5 * n + 1;
    t.ctr = reinterpret_cast<uint32_t *>(buf + 6 * n + 1); t.order = t.ctr + 1;
    t.blk = reinterpret_cast<uint32_t *>(buf + blm_desc_words64(n_clips));
    return t;
}

// one clip's entries once its first unit and its packed output offset are known; the block table gets the clip of every 16th unit
// inside [first_unit, first_unit + units)
MS_BLM_HD void blm_desc_write_clip(const BlmDescTables &t, uint32_t c, uint64_t off, const BlmDescClip &k, uint64_t first_unit, uint64_t out_off,
                                   uint64_t max_blocks) {
    t.off[c] = off; t.frames[c] = k.cols; t.out_off[c] = out_off; t.prefix[c] = first_unit;
    t.len[c] = k.len; t.valid[c] = k.valid;
    for (uint64_t b = (first_unit + kBlmDescUnitBlock - 1) / kBlmDescUnitBlock; b * kBlmDescUnitBlock < first_unit + k.units && b < max_blocks; ++b) t.blk[b] = c;
}
// Rule (B): the columns of the clips that survive (A) sum to more than max_total_columns -- every clip is rejected: a batch of n_clips
// clips of length 0, which launches no unit and no row
MS_BLM_HD BlmDescClip blm_desc_empty_clip() { return BlmDescClip{0, 0, 0, 0, true}; }

// The planner, serially, from host arrays: what blm_plan_ragged_device_kernel writes into `buf` (blm_desc_bytes), and the number of
// rejected clips.  h_out_off may be null: outputs packed in clip order.
inline uint32_t blm_desc_plan_serial(const BlmDescGeom &g, const uint64_t *h_off, const uint64_t *h_len, const uint64_t *h_out_off, uint32_t n_clips,
                                     uint64_t max_total_columns, uint64_t max_clip_samples, uint64_t *buf) {
    const BlmDescTables t = blm_desc_tables(buf, n_clips);
    const uint64_t max_blocks = blm_desc_max_blocks(blm_desc_max_units(max_total_columns, n_clips));
    uint64_t total = 0, longest = 0;
    uint32_t rejected = 0;
    for (uint32_t c = 0; c < n_clips; ++c) {
        const BlmDescClip k = blm_desc_clip(g, h_len[c], max_clip_samples);
        total += k.cols;
        longest = k.valid > longest ? k.valid : longest;
        rejected += k.rejected ? 1u : 0u;
    }
    const bool all = total > max_total_columns;
    uint64_t unit = 0, out = 0;
    for (uint32_t c = 0; c < n_clips; ++c) {
        const BlmDescClip k = all ? blm_desc_empty_clip() : blm_desc_clip(g, h_len[c], max_clip_samples);
        blm_desc_write_clip(t, c, h_off[c], k, unit, h_out_off ? h_out_off[c] : out, max_blocks);
        unit += k.units;
        out += k.cols * g.n_mels;
    }
    t.prefix[n_clips] = unit;
    *t.ctr = 0;
    *t.order = blm_desc_norm_order(all ? 0 : longest);
    return all ? n_clips : rejected;
}

}  // namespace host
}  // namespace melspec
