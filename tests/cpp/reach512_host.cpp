// reach512_host.cpp -- from a config to the kernel it runs, on the host: the tables the create calls build (fbank_tables.hpp), the shape
// the library takes from them (reach512 / shape512, fused512_route.hpp) and route512's kernel per kind of batch.  Nothing observes which
// kernel a GPU call ran; this is the library's own decision code on the configs of tests/test_four_wave.py.  Stand-alone, no HIP, never
// loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -Wno-unknown-pragmas -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/reach512_host.cpp -o /tmp/reach512_host
//   /tmp/reach512_host kaldi:16000:4 nemo:9600:4:slaney whisper:16000:8     one line per config: blob bytes, fused, waves, LDS, kernels
//   /tmp/reach512_host --sweep                                             the two sweeps below, one summary line each (--sweep-coarse: every eighth rate)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fbank_tables.hpp"
#include "fused512_route.hpp"

using namespace melspec;
using namespace melspec::host;

static const char *const kNames[] = {
#define MS_X(name, ...) #name,
    MS_K512_WAVE(MS_X) MS_K512_IO(MS_X) MS_K512_CLIP(MS_X) MS_K512_STATS(MS_X) MS_K512_AUTO(MS_X) MS_K512_STREAM(MS_X)
#undef MS_X
};
static_assert(sizeof(kNames) / sizeof(kNames[0]) == static_cast<int>(K512::kEnd), "one name per K512");
static const char *name_of(K512 k) { return k == K512::kNone ? "kNone" : kNames[static_cast<int>(k)]; }

struct Reached {
    bool tables;             // the bank has the two-filters-per-bin structure the fused kernels need
    size_t blob_bytes;
    Reach512 reach;
    Fused512Shape shape;
};

// melspec_fbank_create: default geometry (25 ms frames at 16 kHz are 400 samples; the tables depend on the rate through the bank alone)
static Reached kaldi(double sr, int bins, double low = 20.0) {
    FbankFastTables ft;
    Reached r{};
    r.tables = build_fbank_fast_tables<double>(sr, bins, low, sr / 2.0, true, ft);
    if (!r.tables) return r;
    r.blob_bytes = ft.blob.size() * 4;
    r.reach = reach512(Flavor512::kKaldi, r.blob_bytes);
    r.shape = shape512<LensKaldi80, LensKaldi40>(Flavor512::kKaldi, r.reach, ft.slots, Bank512::kKaldi80, Bank512::kKaldi40, kFbSlots);
    r.shape.cmn_power = true;
    return r;
}
// melspec_blm_create at n_fft = 512, win_length = 400
static Reached nemo(int sr, int n_mels, bool htk, double f_min = 0.0) {
    FbankFastTables ft;
    Reached r{};
    r.tables = build_blm_fast_tables<double>(sr, n_mels, f_min, sr / 2.0, htk, true, ft);
    if (!r.tables) return r;
    r.blob_bytes = ft.blob.size() * 4;
    r.reach = reach512(Flavor512::kNemo, r.blob_bytes);
    r.shape = shape512<LensSlaney128, LensSlaney80>(Flavor512::kNemo, r.reach, ft.slots, Bank512::kSlaney128, Bank512::kSlaney80, kFbSlots);
    return r;
}
// melspec_create at n_fft = 512: the default bank, or (the sweep) one a caller hands in
static Reached whisper(double sr, int n_mels, bool htk = false, double f_min = -1.0) {
    FbankFastTables ft;
    Reached r{};
    r.tables = build_whisper512_tables<double>(mel_filterbank(sr, 512, n_mels, f_min, -1.0, htk, true), n_mels, ft);
    if (!r.tables) return r;
    r.blob_bytes = ft.blob.size() * 4;
    r.reach = reach512(Flavor512::kWhisper, r.blob_bytes);
    r.shape = shape512<LensSlaney80W, LensSlaney128>(Flavor512::kWhisper, r.reach, ft.slots, Bank512::kSlaney80W, Bank512::kSlaney128, kFbSlots);
    return r;
}

static int bad = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++bad <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                  \
    } while (0)

// what every reached object has to be, whatever the config
static void check(const Reached &r, const char *what, double sr, int n) {
    if (!r.tables) return;
    const Reach512 eight = reach512_at(r.shape.flavor, r.blob_bytes, 8);
    CHECK(r.reach.waves == (eight.fused ? 8 : 4), "%s %g Hz %d bins: %d waves", what, sr, n, r.reach.waves);
    CHECK(!r.reach.fused || r.reach.lds_bytes <= 160 * 1024, "%s %g Hz %d bins: fused with %zu bytes of LDS", what, sr, n, r.reach.lds_bytes);
    CHECK(r.reach.lds_bytes == r.blob_bytes + static_cast<size_t>(r.reach.waves) * (17408 + (r.shape.flavor == Flavor512::kWhisper ? 512 : 0)) +
                                   (r.shape.flavor == Flavor512::kNemo ? 64 : 0), "%s %g Hz %d bins: %zu bytes", what, sr, n, r.reach.lds_bytes);
    // (four waves fit whatever the family's tables are: the largest blob is 37 120 bytes)
    CHECK(r.reach.fused, "%s %g Hz %d bins: a blob of %zu bytes leaves the fused path", what, sr, n, r.blob_bytes);
}

static int one(const char *arg) {
    char flavor[16] = "", bank[16] = "slaney";
    double sr = 0.0;
    int n = 0;
    if (std::sscanf(arg, "%15[a-z]:%lf:%d:%15[a-z]", flavor, &sr, &n, bank) < 3) { std::printf("FAILED to read %s\n", arg); return 1; }
    const bool htk = !std::strcmp(bank, "htk");
    Reached r;
    if (!std::strcmp(flavor, "kaldi")) r = kaldi(sr, n);
    else if (!std::strcmp(flavor, "nemo")) r = nemo(static_cast<int>(sr), n, htk);
    else if (!std::strcmp(flavor, "whisper")) r = whisper(sr, n);
    else { std::printf("FAILED to read %s\n", arg); return 1; }
    if (!r.tables) { std::printf("%s tables=0\n", arg); return 0; }
    check(r, flavor, sr, n);
    const int s16_f16 = MELSPEC_PCM_S16 | MELSPEC_OUT_F16 << 4;
    std::printf("%s tables=1 blob=%zu fused=%d waves=%d lds=%zu plain=%s layout=%s stream=%s clip=%s clip_ragged=%s io=%s stats=%s clip_shape_ok=%d\n", arg, r.blob_bytes,
                r.reach.fused ? 1 : 0, r.reach.waves, r.reach.lds_bytes, name_of(route512(r.shape, Batch512::kPlain).run.kernel),
                name_of(route512(r.shape, Batch512::kLayout).run.kernel), name_of(route512(r.shape, Batch512::kStream).run.kernel),
                name_of(route512(r.shape, Batch512::kClipUniform).run.kernel), name_of(route512(r.shape, Batch512::kClipRagged).run.kernel),
                name_of(route512(r.shape, Batch512::kIo, s16_f16).run.kernel), name_of(route512(r.shape, Batch512::kStats).run.kernel),
                clip_shape_ok(r.shape, n) ? 1 : 0);
    return 0;
}

// (a) few, wide filters: NeMo banks of 1 .. 16 mels at 4 .. 48 kHz, Slaney and HTK.  A blob of exactly 24 576 bytes fits eight slices but
//     not eight slices and the RoundSync counters: such an object runs on four waves, fused (the rule used to ask without the counters,
//     say "eight", and the object left the fused path 64 bytes over).
// (b) many, narrow filters: 90 .. 149 mels at 4 .. 96 kHz, Slaney and HTK, f_min 0 and 50 Hz, the NeMo frontend and Whisper at
//     n_fft = 512: no such bank is on four waves, so kNemoRt10x4 and kWRt10x4 are not reachable in a product build.
static void sweep(int coarse) {
    long n_few = 0, holes = 0, four_few = 0;
    for (int sr = 4000; sr <= 48000; sr += 50 * coarse)
        for (int n = 1; n <= 16; ++n)
            for (int htk = 0; htk < 2; ++htk) {
                const Reached r = nemo(sr, n, htk != 0);
                if (!r.tables) continue;
                ++n_few;
                check(r, "nemo", sr, n);
                four_few += r.reach.waves == 4;
                if (r.blob_bytes == 24576) {
                    ++holes;
                    CHECK(r.reach.fused && r.reach.waves == 4 && route512(r.shape, Batch512::kLayout).run.kernel == K512::kNemoRt6x4, "nemo %d Hz %d mels: a 24 576-byte blob", sr, n);
                }
                CHECK(r.shape.small_slots, "nemo %d Hz %d mels: more than six slots", sr, n);
            }
    std::printf("sweep few: configs=%ld four_wave=%ld holes=%ld\n", n_few, four_few, holes);
    long n_many = 0, ten_x4 = 0, four_many = 0;
    size_t largest = 0;
    for (int sr = 4000; sr <= 96000; sr += 1000 * coarse)
        for (int n = 90; n <= 149; ++n)
            for (int htk = 0; htk < 2; ++htk)
                for (int lo = 0; lo < 2; ++lo) {
                    const Reached rs[2] = {nemo(sr, n, htk != 0, lo ? 50.0 : 0.0), whisper(sr, n, htk != 0, lo ? 50.0 : -1.0)};
                    for (const Reached &r : rs) {
                        if (!r.tables) continue;
                        ++n_many;
                        check(r, r.shape.flavor == Flavor512::kNemo ? "nemo" : "whisper", sr, n);
                        if (r.blob_bytes > largest) largest = r.blob_bytes;
                        four_many += r.reach.waves == 4;
                        for (Batch512 kind : {Batch512::kPlain, Batch512::kLayout}) {
                            const K512 k = route512(r.shape, kind).run.kernel;
                            ten_x4 += k == K512::kNemoRt10x4 || k == K512::kWRt10x4;
                        }
                    }
                }
    std::printf("sweep many: configs=%ld four_wave=%ld ten_slot_four_wave=%ld largest_blob=%zu\n", n_many, four_many, ten_x4, largest);
}

int main(int argc, char **argv) {
    int rc = 0;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--sweep")) sweep(1);
        else if (!std::strcmp(argv[i], "--sweep-coarse")) sweep(8);          // every eighth rate: the sanitized build's
        else rc |= one(argv[i]);
    }
    if (bad) std::printf("FAILED (%d checks)\n", bad);
    else if (!rc) std::printf("reach512_host: ok\n");
    return bad || rc ? 1 : 0;
}
