"""The auxiliary device entry points, whole batch: every image, frame and value against the oracle, in fenced output buffers.

melspec_vad_boundaries_device, melspec_tga_encode_device / _decode_device, melspec_quantize_device / _dequantize_device and
melspec_bank_project_power_device / _log_mel_device / _norm_mel_device were reached only through their `_host` forms (one image, tight
strides, the object's own stream) or through one batched test that sampled 4 images of 48.  Here each of them is called through its
Python mirror with more than one image (or frame, or grid-stride pass), strides larger than the payload, once on the object's own
stream and once on a caller's, and writes into the middle of an allocation filled with a sentinel: the NaN word 0x7fc0dead of
tests/test_whole_batch.py for floats, the byte 0xA5 for masks and blobs.  check_fenced asserts, on the whole allocation,
  (a) both guard bands are intact,
  (b) every gap a stride leaves between two outputs still holds the sentinel,
  (c) no sentinel is left where a value belongs,
  (d) every value equals the oracle's (bit for bit, except log_mel, which has the tolerance of test_sparse_filterbank_helpers).
The failing direction of check_fenced is exercised on doctored numpy arrays (test_check_fenced_rejects_doctored_arrays).

VAD masks.  On N(0, 1) images taller than a few rows the raw mask is all ones under the settings tests/test_vad.py used, so the Sobel
walk's count, its early exit and the eight-row batching were compared with "all true".  The two `mixed` settings per height below give
a raw-mask share of ones inside [0.10, 0.90] on the noise images; test_vad_mixed_settings_give_mixed_masks asserts it on the oracle.
Measured on the oracle for the noise images (image 0, image 4) of vad_images():
    rows  settings (min_energy, min_y, min_mel)   width 258     width 259     width 700
      80  (6.0, 20, 0)                            0.25, 0.35    0.24, 0.28    0.31, 0.33
      80  (7.0, 12, 2)                            0.30, 0.30    0.28, 0.31    0.29, 0.35
     128  (6.0, 30, 0)                            0.39, 0.48    0.39, 0.39    0.43, 0.42
     128  (7.0, 18, 2)                            0.36, 0.42    0.36, 0.38    0.38, 0.38
(at 128 rows the 80-row settings give 0.93 .. 0.96 and 0.80 .. 0.88: min_y is raised until the share is back in the middle of the band).

NaN payloads: where the oracle's dequantised value is a NaN (the image whose range is {-inf, +inf}: 0 * inf), the device value must be
a NaN too; IEEE 754 leaves sign and payload of a generated NaN open, and the x86 host and the GPU choose differently."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py): device properties and caller streams come from here

from conftest import ROOT
from test_whole_batch import GUARD, SENTINEL, Fence, _upload

BYTE_SENTINEL = np.uint8(0xA5)
BYTE_GUARD = 8192                                        # bytes of guard band on each side of a mask / blob output
SENTINEL64 = np.uint64((int(SENTINEL) << 32) | int(SENTINEL))
TGA_HEADER, TGA_MAX_W = 26, 65535


# ---- the comparison helper (pure numpy: the CPU tests below run it on the emulation's output and on doctored arrays) ----------------

def check_fenced(raw, guard, items, sentinel, what, zero_ok=(), tol=None, nan_equal=False):
    """raw: a whole fenced allocation as it came back -- `guard` elements of guard band, the output region, `guard` elements again.
    items: [(offset into the region, expected array of raw's dtype)]; everything of the region no item covers is a gap.  zero_ok:
    region indices of gap elements that may hold 0 instead of the sentinel.  tol: compare as floats of the expected dtype within tol
    instead of bit for bit.  nan_equal (uint32 words of f32 values): a NaN where the expected value is a NaN counts as equal.
    -> the items' values as found."""
    raw = np.asarray(raw)
    s = raw.dtype.type(sentinel)
    n = raw.size - 2 * guard
    assert n >= 0
    lo, body, hi = raw[:guard], raw[guard:guard + n], raw[guard + n:]
    assert np.all(lo == s), f"{what}: write below the output, {int(np.sum(lo != s))} guard elements changed (last at -{guard - int(np.flatnonzero(lo != s)[-1])})"
    assert np.all(hi == s), f"{what}: write past the output, {int(np.sum(hi != s))} guard elements changed (first at +{int(np.argmax(hi != s))})"
    covered = np.zeros(n, bool)
    found = []
    for k, (off, want) in enumerate(items):
        want = np.asarray(want)
        m = want.size if tol is None else want.size * want.dtype.itemsize // raw.dtype.itemsize
        assert 0 <= off and off + m <= n and not covered[off:off + m].any(), (what, k, off, m, n)
        covered[off:off + m] = True
        g = body[off:off + m]
        if tol is None:
            assert want.dtype == raw.dtype, (want.dtype, raw.dtype)
            left = (g == s) & (want != s)
            assert not left.any(), f"{what}: item {k}: {int(left.sum())} elements never written (first at {int(np.argmax(left))})"
            same = g == want
            if nan_equal:
                same |= np.isnan(g.view(np.float32)) & np.isnan(want.view(np.float32))
            assert same.all(), f"{what}: item {k}: {int((~same).sum())} of {m} elements differ from the oracle, first at " \
                               f"{int(np.argmax(~same))}: {g[int(np.argmax(~same))]:#x} != {want[int(np.argmax(~same))]:#x}"
        else:
            left = g == s
            assert not left.any(), f"{what}: item {k}: {int(left.sum())} elements never written (first at {int(np.argmax(left))})"
            d = np.abs(g.view(want.dtype).astype(np.float64) - want.astype(np.float64).ravel())
            d[np.isnan(d)] = np.inf
            assert d.max() <= tol, f"{what}: item {k}: |diff| {d.max():.3e} > {tol:.1e} at {int(np.argmax(d))}"
        found.append(g)
    soft = np.zeros(n, bool)
    if len(zero_ok):
        soft[np.asarray(zero_ok, np.int64)] = True
    bad = ~covered & (body != s) & ~(soft & (body == 0))
    assert not bad.any(), f"{what}: {int(bad.sum())} gap elements changed (first at {int(np.argmax(bad))}: {body[int(np.argmax(bad))]:#x})"
    return found


def longest_run(mask):
    return max(len(r) for r in "".join("1" if b else "0" for b in mask).split("0"))


def _u8(a):
    return np.ascontiguousarray(a).astype(np.uint8) if np.asarray(a).dtype == bool else np.ascontiguousarray(a).view(np.uint8).ravel()


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32).ravel()


# ---- fenced device buffers ---------------------------------------------------------------------------------------------------------

class ByteFence:
    """Fence's sibling for masks and blobs: n bytes inside an allocation of n + 2 BYTE_GUARD bytes, all of it 0xA5 before the call."""

    def __init__(self, gpu, n):
        self.n = int(n)
        self.buf = gpu.DeviceBuffer(self.n + 2 * BYTE_GUARD)
        self.buf.upload(np.full(self.n + 2 * BYTE_GUARD, BYTE_SENTINEL, np.uint8))
        self.ptr = self.buf.ptr + BYTE_GUARD

    def raw(self):
        r = self.buf.download(self.n + 2 * BYTE_GUARD, np.uint8)
        self.buf.free()
        return r


def fence_raw(f, dtype=np.uint32):
    """the whole allocation of a Fence (tests/test_whole_batch.py), guard bands included, as uint32 or uint64 words"""
    r = f.buf.download(f.n + 2 * GUARD, np.uint32)
    f.buf.free()
    return r if dtype == np.uint32 else r.view(np.uint64)


def check_bytes(f, items, what, zero_ok=()):
    return check_fenced(f.raw(), BYTE_GUARD, items, BYTE_SENTINEL, what, zero_ok)


def check_words(f, items, what, nan_equal=False):
    return check_fenced(fence_raw(f), GUARD, items, SENTINEL, what, nan_equal=nan_equal)


def check_doubles(f, items, what, tol=None):
    return check_fenced(fence_raw(f, np.uint64), GUARD // 2, items, SENTINEL64, what, tol=tol)


def _streams():
    """(label, torch stream or None): the object's own stream (null argument), then a caller's"""
    return (("own stream", None), ("caller's stream", torch.cuda.Stream()))


def _sp(stream):
    return None if stream is None else stream.cuda_stream


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


# =====================================================================================================================================
# VAD
# =====================================================================================================================================

VAD_IMAGES = 5
VAD_HEIGHTS = (80, 128)
VAD_WIDTHS = (3, 258, 259, 700)          # n = 1; 256: exactly one block per image; 257: a second block with one thread; 698: three blocks
VAD_MIXED = {80: (dict(min_energy=6.0, min_y=20, min_mel=0), dict(min_energy=7.0, min_y=12, min_mel=2)),
             128: (dict(min_energy=6.0, min_y=30, min_mel=0), dict(min_energy=7.0, min_y=18, min_mel=2))}
VAD_NOISE, VAD_CONST, VAD_HALF, VAD_RUN = (0, 4), 1, 2, 3


def vad_settings(h):
    """the defaults; min_y = 0 (everything set); min_mel beyond the image (nothing set); the two mixed-mask settings of this height"""
    return (dict(min_energy=0.98, min_y=11, min_mel=2), dict(min_energy=0.98, min_y=0, min_mel=2), dict(min_energy=0.98, min_y=11, min_mel=200)) + VAD_MIXED[h]


def vad_run_band(w):
    """image columns of the busy band of the `run` image: some way in, longer than three lane pieces of vad_run_kernel"""
    n = max(w - 2, 1)
    per = (n + 63) // 64
    c0 = w // 5 + 1
    c1 = min(w, c0 + 3 * per + per // 2 + 6)
    if per > 1:                              # mask columns c0 - 2 .. c1 - 1 are set: both ends inside a piece
        c0 += (c0 - 2) % per == 0
        c1 += c1 % per == 0
    return c0, c1


@functools.lru_cache(maxsize=None)
def vad_images(h, w):
    """[noise, constant, noise on the left half and constant on the right, constant but for one busy band of columns, noise]"""
    def noise(seed):
        return np.random.default_rng(seed * 100003 + h * 1009 + w).standard_normal((h, w)).astype(np.float32)
    half = noise(2)
    half[:, w // 2:] = np.float32(-1.25)
    run = np.full((h, w), 0.5, np.float32)
    c0, c1 = vad_run_band(w)
    run[:, c0:c1] = 100.0 * noise(3)[:, c0:c1]
    imgs = [noise(1), np.full((h, w), 0.37, np.float32), half, run, noise(4)]
    for a in imgs:
        a.setflags(write=False)
    return tuple(imgs)


@functools.lru_cache(maxsize=None)
def vad_want(h, w, kw):
    """per image (raw mask, smoothed mask, longest run of the smoothed mask), from the oracle"""
    O = _oracle()
    out = []
    for img in vad_images(h, w):
        raw, sm = O.vad_boundaries(img, **dict(kw))
        out.append((raw, sm, longest_run(sm)))
    return out


def _kw_key(kw):
    return tuple(sorted(kw.items()))


def test_vad_mixed_settings_give_mixed_masks():
    """On the oracle alone: the two mixed settings of each height leave the raw masks of the noise images between 10 % and 90 % ones,
    the constant image has no column set, the half-constant image is mixed, min_y = 0 sets every column, min_mel = 200 none, and the
    `run` image's smoothed mask is one run longer than a lane piece of vad_run_kernel that starts and ends inside pieces."""
    for h in VAD_HEIGHTS:
        for w in VAD_WIDTHS[1:]:
            n = w - 2
            per = (n + 63) // 64
            dflt, every, none = vad_settings(h)[:3]
            for kw in VAD_MIXED[h]:
                want = vad_want(h, w, _kw_key(kw))
                for i in VAD_NOISE:
                    share = float(want[i][0].mean())
                    print(f"rows {h} width {w} {kw}: image {i} raw share {share:.3f}")
                    assert 0.10 <= share <= 0.90, (h, w, kw, i, share)
                assert not want[VAD_CONST][0].any() and want[VAD_CONST][2] == 0
                hr = want[VAD_HALF][0]
                assert hr[:n // 2 - 2].any() and not hr[n // 2 + 2:].any()
            for kw in (dflt,) + VAD_MIXED[h]:
                sm = vad_want(h, w, _kw_key(kw))[VAD_RUN][1]
                on = np.flatnonzero(sm)
                assert on.size == on[-1] - on[0] + 1 == vad_want(h, w, _kw_key(kw))[VAD_RUN][2], "one run"
                assert on.size > per and on[0] // per + 2 <= on[-1] // per, "the run spans lane pieces"
                assert on[0] % per != 0 and (on[-1] + 1) % per != 0, "the run starts and ends inside a piece"
            assert all(r.all() and s.all() and run == n for r, s, run in vad_want(h, w, _kw_key(every)))
            assert n % 64 != 0 or w == 258
            assert all(not r.any() and not s.any() and run == 0 for r, s, run in vad_want(h, w, _kw_key(none)))


def _vad_call(gpu, h, w, kw, tight, stream, with_run=True):
    """one melspec_vad_boundaries_device call over the five images of (h, w) -> the three fences, checked against the oracle"""
    n = w - 2
    px = h * w
    istride, mstride = (px, n) if tight else (px + 7, n + 5)
    host = np.full(VAD_IMAGES * istride, 1e30, np.float32)                  # a read of a gap float would set a column
    for i, img in enumerate(vad_images(h, w)):
        host[i * istride:i * istride + px] = img.ravel()
    d = _upload(gpu, host)
    raw, sm, run = ByteFence(gpu, VAD_IMAGES * mstride), ByteFence(gpu, VAD_IMAGES * mstride), Fence(gpu, VAD_IMAGES)
    gpu.vad_boundaries_device(d.ptr, istride, h, w, VAD_IMAGES, gpu.DetectionSettings(**kw), raw.ptr, sm.ptr, mstride,
                              run.ptr if with_run else None, stream=_sp(stream))
    gpu.device_synchronize()
    want = vad_want(h, w, _kw_key(kw))
    what = f"vad {h}x{w} {kw} {'tight' if tight else 'strided'} ({'null stream' if stream is None else 'a caller stream'})"
    check_bytes(raw, [(i * mstride, _u8(want[i][0])) for i in range(VAD_IMAGES)], what + ": raw mask")
    check_bytes(sm, [(i * mstride, _u8(want[i][1])) for i in range(VAD_IMAGES)], what + ": smoothed mask")
    check_words(run, [(0, np.array([wi[2] for wi in want], np.uint32))] if with_run else [], what + ": longest_run")
    d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("h", VAD_HEIGHTS)
@pytest.mark.parametrize("w", VAD_WIDTHS)
def test_gpu_vad_batch_every_column_of_every_image(gpu, h, w):
    """Five images per call (image index > 0 in all three kernels), image_stride = n_mels * width + 7 with 1e30 in the gaps,
    mask_stride = n + 5, under the five settings, on the null stream and on a caller's; one run with both strides tight; one without
    d_longest_run (the masks are the same, the words where the runs would go keep the sentinel)."""
    for _, stream in _streams():
        for kw in vad_settings(h):
            _vad_call(gpu, h, w, kw, False, stream)
    _vad_call(gpu, h, w, vad_settings(h)[3], True, None)
    _vad_call(gpu, h, w, vad_settings(h)[4], True, torch.cuda.Stream())
    _vad_call(gpu, h, w, vad_settings(h)[3], False, None, with_run=False)


@pytest.mark.gpu
def test_gpu_vad_refusals_and_empty_masks(gpu):
    """mask_stride < n, image_stride < n_mels * width and a null d_raw are refused with nothing written; n_mels < 3 or width < 3 zeroes
    d_longest_run for every image and writes no mask byte."""
    h, w = 80, 259
    n, px = w - 2, h * w
    d = _upload(gpu, np.concatenate([img.ravel() for img in vad_images(h, w)]))
    st = gpu.DetectionSettings()
    for label, stream in _streams():
        for what, istride, mstride, null_raw in (("mask_stride < n", px, n - 1, False), ("image_stride < n_mels * width", px - 1, n, False),
                                                 ("null d_raw", px, n, True)):
            raw, sm, run = ByteFence(gpu, VAD_IMAGES * n), ByteFence(gpu, VAD_IMAGES * n), Fence(gpu, VAD_IMAGES)
            with pytest.raises(gpu.HipRuntimeError):
                gpu.vad_boundaries_device(d.ptr, istride, h, w, VAD_IMAGES, st, None if null_raw else raw.ptr, sm.ptr, mstride, run.ptr, stream=_sp(stream))
            gpu.device_synchronize()
            check_bytes(raw, [], what + ": raw mask"); check_bytes(sm, [], what + ": smoothed mask"); check_words(run, [], what + ": longest_run")
        for hh, ww in ((2, 259), (80, 2), (0, 0)):
            raw, sm, run = ByteFence(gpu, 64), ByteFence(gpu, 64), Fence(gpu, VAD_IMAGES + 3)
            gpu.vad_boundaries_device(d.ptr, hh * ww, hh, ww, VAD_IMAGES, st, raw.ptr, sm.ptr, 8, run.ptr + 4, stream=_sp(stream))
            gpu.device_synchronize()
            what = f"empty mask {hh}x{ww} ({label})"
            check_bytes(raw, [], what + ": raw mask"); check_bytes(sm, [], what + ": smoothed mask")
            check_words(run, [(1, np.zeros(VAD_IMAGES, np.uint32))], what + ": longest_run")
    d.free()


# =====================================================================================================================================
# TGA container and the bare quantiser
# =====================================================================================================================================

def tga_layout(rows, width):
    """(chunks, columns of a full chunk, chunk_stride, [bytes of chunk c]): melspec_tga_layout restated"""
    chunks = (width + TGA_MAX_W - 1) // TGA_MAX_W
    cw = min(width, TGA_MAX_W)
    stride = (TGA_HEADER + rows * cw + 3) & ~3
    return chunks, cw, stride, [TGA_HEADER + rows * min(cw, width - c * cw) for c in range(chunks)]


@functools.lru_cache(maxsize=None)
def quant_images(rows, width, n_images):
    """Images whose ranges differ by orders of magnitude (1e-3, 1, 1e3, ...; the columns of a second chunk another 1e2), image 1 with
    a NaN, a +inf and a -inf pixel, the last image constant: a key slot taken from a neighbour shows in the header and in every byte."""
    px = rows * width
    imgs = []
    for i in range(n_images):
        x = np.random.default_rng(7000 + i + rows * 31 + width).standard_normal((rows, width)).astype(np.float32) * np.float32(10.0 ** (3 * i - 3))
        x[:, TGA_MAX_W:] *= np.float32(100.0)
        imgs.append(x)
    flat = imgs[1].reshape(-1)
    flat[px // 3], flat[px // 2], flat[(2 * px) // 3] = np.nan, np.inf, -np.inf
    imgs[-1][:] = np.float32(-2.5)
    for a in imgs:
        a.setflags(write=False)
    return tuple(imgs)


@functools.lru_cache(maxsize=None)
def quant_want(rows, width, n_images):
    """per image: (the oracle's blobs, one per chunk; the image parse_tga_8bit gives back from them)"""
    O = _oracle()
    chunks, cw, _, sizes = tga_layout(rows, width)
    out = []
    for img in quant_images(rows, width, n_images):
        blobs = O.tga_8bit(img, rows)
        assert [len(b) for b in blobs] == sizes
        back = np.empty((rows, width), np.float32)
        for c, b in enumerate(blobs):
            back[:, c * cw:c * cw + (len(b) - TGA_HEADER) // rows] = O.parse_tga_8bit(b).reshape(rows, -1)
        out.append((blobs, back))
    ranges = {bytes(b[18:26]) for blobs, _ in out for b in blobs}
    assert len(ranges) == (len(out) - 1) * chunks + 1, "every item has a range of its own (the constant image one for all its chunks)"
    return out


# (rows, width, images, floats between images beyond the payload, bytes between blobs beyond the layout, image pointer moved by bytes)
TGA_CASES = {
    "a-vector": (80, 333, 5, 0, 8, 0),                    # tight, 16-byte aligned images: the vector path
    "b-odd-stride": (80, 333, 5, 1, 8, 0),                # image_stride % 4 != 0: the scalar path in a batch
    "b-moved-pointer": (80, 333, 5, 0, 8, 4),             # the image pointer not 16-byte aligned: the scalar path in a batch
    "c-two-chunks": (3, 65541, 3, 2, 4, 0),               # item / chunks with more than one image
    "d-1x7": (1, 7, 5, 1, 8, 0),
    "d-80x1": (80, 1, 5, 1, 8, 0),
}


def tga_plan(case):
    rows, width, n_images, img_gap, blob_gap, shift = TGA_CASES[case]
    chunks, cw, cstride, sizes = tga_layout(rows, width)
    return dict(rows=rows, width=width, n_images=n_images, shift=shift, chunks=chunks, cstride=cstride, sizes=sizes,
                istride=rows * width + img_gap, bstride=chunks * cstride + blob_gap)


def tga_host_images(p, gap=1e30):
    """the images at their stride, 1e30 (or `gap`) in the floats between them: a read of one would take over the range"""
    host = np.full(p["n_images"] * p["istride"], gap, np.float32)
    for i, img in enumerate(quant_images(p["rows"], p["width"], p["n_images"])):
        host[i * p["istride"]:i * p["istride"] + img.size] = img.ravel()
    return host


def tga_blob_items(p):
    """-> (items, zero_ok) of the blob region: every chunk of every image; the bytes up to the next multiple of four behind a chunk are
    written as zeros by an encoder that stores whole dwords"""
    items, soft = [], []
    for i, (blobs, _) in enumerate(quant_want(p["rows"], p["width"], p["n_images"])):
        for c, b in enumerate(blobs):
            off = i * p["bstride"] + c * p["cstride"]
            items.append((off, np.frombuffer(b, np.uint8)))
            soft += list(range(off + len(b), (off + len(b) + 3) & ~3))
    return items, soft


def tga_host_blobs(p):
    """the oracle's blobs at their strides, the sentinel byte everywhere else"""
    host = np.full(p["n_images"] * p["bstride"], BYTE_SENTINEL, np.uint8)
    for off, b in tga_blob_items(p)[0]:
        host[off:off + b.size] = b
    return host


def tga_image_items(p, lead=0):
    return [(lead + i * p["istride"], _u32(back)) for i, (_, back) in enumerate(quant_want(p["rows"], p["width"], p["n_images"]))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(TGA_CASES))
def test_gpu_tga_batch_every_byte_of_every_blob(gpu, case):
    """melspec_tga_encode_device: every chunk of every image byte for byte against tga_8bit_data, the blob gaps untouched.
    melspec_tga_decode_device on the oracle's blobs: every pixel bit for bit against parse_tga_8bit, the image gaps untouched."""
    p = tga_plan(case)
    codec = gpu.TgaCodec()
    n, st, last = codec.layout(p["rows"], p["width"])
    assert (n, st, last) == (p["chunks"], p["cstride"], p["sizes"][-1])
    shift = p["shift"]
    src = gpu.DeviceBuffer(p["n_images"] * p["istride"] * 4 + 16)
    src.upload(tga_host_images(p), shift)
    assert src.ptr % 16 == 0
    d_blobs = _upload(gpu, tga_host_blobs(p))
    items, soft = tga_blob_items(p)
    for label, stream in _streams():
        what = f"tga {case} ({label})"
        out = ByteFence(gpu, p["n_images"] * p["bstride"])
        codec.encode_device(src.ptr + shift, p["istride"], p["rows"], p["width"], p["n_images"], out.ptr, p["bstride"], stream=_sp(stream))
        gpu.device_synchronize()
        check_bytes(out, items, what + ": encode", soft)
        back = Fence(gpu, p["n_images"] * p["istride"] + shift // 4)
        codec.decode_device(d_blobs.ptr, p["bstride"], p["rows"], p["width"], p["n_images"], back.ptr + shift, p["istride"], stream=_sp(stream))
        gpu.device_synchronize()
        check_words(back, tga_image_items(p, shift // 4), what + ": decode", nan_equal=True)
    src.free(); d_blobs.free(); codec.close()


def _quant_input(n, with_nan):
    x = (np.random.default_rng(9000 + n).standard_normal(n) * 3).astype(np.float32)
    if with_nan:
        x[n // 2] = np.nan
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 1001, 2 * 16384 + 5])
def test_gpu_bare_quantiser_device_calls(gpu, n):
    """melspec_quantize_device / melspec_dequantize_device (no container): the bytes, the two range floats and the dequantised floats
    bit for bit against quantize / dequantize, with the float pointer 16-byte aligned (vector loads) and moved by 4 bytes (scalar)."""
    O = _oracle()
    codec = gpu.TgaCodec()
    n4 = (n + 3) & ~3
    for with_nan in (False, True):
        x = _quant_input(n, with_nan)
        q, r = O.quantize(x)
        r = np.asarray(r, np.float32)
        deq = O.dequantize(q, r)
        d_q = _upload(gpu, np.concatenate([q, np.full(n4 - n, BYTE_SENTINEL, np.uint8)]))
        d_r = _upload(gpu, r)
        for shift in (0, 4):
            src = gpu.DeviceBuffer(n * 4 + 16)
            src.upload(x, shift)
            assert src.ptr % 16 == 0
            for label, stream in _streams():
                what = f"quantize n={n} nan={with_nan} shift={shift} ({label})"
                out, rng = ByteFence(gpu, n4), Fence(gpu, 2)
                codec.quantize_device(src.ptr + shift, n, out.ptr, rng.ptr, stream=_sp(stream))
                gpu.device_synchronize()
                check_bytes(out, [(0, q)], what + ": bytes", list(range(n, n4)))
                check_words(rng, [(0, _u32(r))], what + ": range")
                back = Fence(gpu, n + shift // 4)
                codec.dequantize_device(d_q.ptr, n, d_r.ptr, back.ptr + shift, stream=_sp(stream))
                gpu.device_synchronize()
                check_words(back, [(shift // 4, _u32(deq))], what + ": dequantised", nan_equal=True)      # n = 1, a NaN: the range is {inf, -inf}
            src.free()
        d_q.free(); d_r.free()
    codec.close()


# ---- the same batches through the kernels' per-thread functions on the host (tests/emu) ---------------------------------------------

@pytest.fixture(scope="module")
def qemu():
    d = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libmelspec_emu.so"))
    vp = C.c_void_p
    L.emu_tga_encode.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, vp, C.c_uint64, C.c_int, vp]
    L.emu_tga_decode.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, vp, C.c_uint64, C.c_int, vp]
    return L


def _placed(values, mod16, lead, tail, fill):
    """a copy of `values` inside a larger array of `fill`, `lead` elements in, with its first element at an address == mod16 (mod 16)
    -> (the owner, the whole fenced view [lead + n + tail], the address of the values)"""
    v = np.ascontiguousarray(values)
    it = v.dtype.itemsize
    own = np.full(lead + v.size + tail + 32 // it, fill, v.dtype)
    k = next(k for k in range(32 // it) if (own.ctypes.data + (k + lead) * it) % 16 == mod16)
    view = own[k:k + lead + v.size + tail]
    view[lead:lead + v.size] = v
    return own, view, view.ctypes.data + lead * it


@pytest.mark.parametrize("case", ["b-odd-stride", "b-moved-pointer", "c-two-chunks"])
def test_emulated_tga_batches_with_strides(qemu, case):
    """Cases (b) and (c) through encode_dword / decode_dword on the host (emu_tga_encode / emu_tga_decode take n_images and both
    strides): the same blobs, the same pixels, the same gap rules as on the device."""
    p = tga_plan(case)
    shift = p["shift"]
    items, soft = tga_blob_items(p)
    own_src, _, src = _placed(tga_host_images(p), shift, 0, 0, np.float32(0))
    blob_n = p["n_images"] * p["bstride"]
    own_b, out, out_ptr = _placed(np.full(blob_n, BYTE_SENTINEL, np.uint8), 0, BYTE_GUARD, BYTE_GUARD, BYTE_SENTINEL)
    assert qemu.emu_tga_encode(src, p["rows"], p["width"], p["n_images"], p["istride"], out_ptr, p["bstride"], 1, None) == p["n_images"] * p["chunks"]
    check_fenced(out, BYTE_GUARD, items, BYTE_SENTINEL, f"emulated tga {case}: encode", soft)
    own_s, _, blobs_ptr = _placed(tga_host_blobs(p), 0, 0, 0, BYTE_SENTINEL)
    img_n = p["n_images"] * p["istride"]
    own_i, back, back_ptr = _placed(np.full(img_n, SENTINEL, np.uint32), shift, GUARD, GUARD, SENTINEL)
    assert qemu.emu_tga_decode(blobs_ptr, p["bstride"], p["rows"], p["width"], p["n_images"], back_ptr, p["istride"], 1, None) == p["n_images"] * p["chunks"]
    check_fenced(back, GUARD, tga_image_items(p), SENTINEL, f"emulated tga {case}: decode", nan_equal=True)


def test_check_fenced_rejects_doctored_arrays():
    """The failing direction of the comparison helper, on numpy arrays: a clean layout passes; one flipped mask byte, one changed gap
    byte, one changed guard word, one sentinel left in a payload each fail -- for the byte fences and for the word fences."""
    rng = np.random.default_rng(12)
    n, stride, imgs = 257, 262, 5
    masks = [(rng.random(n) < 0.4).astype(np.uint8) for _ in range(imgs)]
    clean = np.full(2 * BYTE_GUARD + imgs * stride, BYTE_SENTINEL, np.uint8)
    for i, m in enumerate(masks):
        clean[BYTE_GUARD + i * stride:BYTE_GUARD + i * stride + n] = m
    items = [(i * stride, m) for i, m in enumerate(masks)]
    check_fenced(clean, BYTE_GUARD, items, BYTE_SENTINEL, "clean")
    soft = list(range(n, n + 3))
    ok = clean.copy(); ok[BYTE_GUARD + n:BYTE_GUARD + n + 3] = 0
    check_fenced(ok, BYTE_GUARD, items, BYTE_SENTINEL, "dword tail", soft)               # zeros where zero_ok allows them
    doctored = {
        "flipped mask byte": (BYTE_GUARD + 3 * stride + 100, None),
        "changed gap byte": (BYTE_GUARD + 2 * stride + n + 1, 0),
        "gap byte changed to something else where a zero would pass": (BYTE_GUARD + n + 1, 1),
        "changed guard byte below": (BYTE_GUARD - 1, 0),
        "changed guard byte above": (BYTE_GUARD + imgs * stride, 1),
        "sentinel left in a payload": (BYTE_GUARD + 4 * stride + n - 1, BYTE_SENTINEL),
    }
    for what, (at, value) in doctored.items():
        bad = clean.copy()
        bad[at] = bad[at] ^ 1 if value is None else value
        with pytest.raises(AssertionError):
            check_fenced(bad, BYTE_GUARD, items, BYTE_SENTINEL, what, soft)
    with pytest.raises(AssertionError):
        check_fenced(ok, BYTE_GUARD, items, BYTE_SENTINEL, "zeros in a gap without leave")
    # words: f32 values (bit for bit), f64 values (tolerance)
    vals = [rng.standard_normal(33).astype(np.float32) for _ in range(3)]
    cleanw = np.full(2 * GUARD + 3 * 40, SENTINEL, np.uint32)
    for i, v in enumerate(vals):
        cleanw[GUARD + i * 40:GUARD + i * 40 + 33] = v.view(np.uint32)
    itemsw = [(i * 40, v.view(np.uint32)) for i, v in enumerate(vals)]
    check_fenced(cleanw, GUARD, itemsw, SENTINEL, "clean words")
    for what, at, value in (("last bit of a value", GUARD + 45, None), ("gap word", GUARD + 35, 0), ("guard word below", 7, 0),
                            ("guard word above", GUARD + 120 + 9, 0), ("sentinel in a payload", GUARD + 80, SENTINEL)):
        bad = cleanw.copy()
        bad[at] = bad[at] ^ 1 if value is None else value
        with pytest.raises(AssertionError):
            check_fenced(bad, GUARD, itemsw, SENTINEL, what)
    nanw = cleanw.copy(); nanw[GUARD + 2] = 0x7FC00000
    wantn = [(o, v.copy()) for o, v in itemsw]; wantn[0][1][2] = 0xFFC00000
    check_fenced(nanw, GUARD, wantn, SENTINEL, "a NaN for a NaN", nan_equal=True)
    with pytest.raises(AssertionError):
        check_fenced(nanw, GUARD, wantn, SENTINEL, "a NaN for a NaN, bit for bit")
    with pytest.raises(AssertionError):
        check_fenced(nanw, GUARD, itemsw, SENTINEL, "a NaN for a number", nan_equal=True)
    d = rng.standard_normal(16)
    cleand = np.full(GUARD + 20, SENTINEL64, np.uint64)
    cleand[GUARD // 2:GUARD // 2 + 16] = d.view(np.uint64)
    check_fenced(cleand, GUARD // 2, [(0, d + 5e-13)], SENTINEL64, "doubles within 1e-12", tol=1e-12)
    with pytest.raises(AssertionError):
        check_fenced(cleand, GUARD // 2, [(0, d + 2e-12)], SENTINEL64, "doubles off by 2e-12", tol=1e-12)
    bad = cleand.copy(); bad[GUARD // 2 + 5] = SENTINEL64
    with pytest.raises(AssertionError):
        check_fenced(bad, GUARD // 2, [(0, d)], SENTINEL64, "sentinel in a payload of doubles", tol=1e-12)
    assert longest_run(np.array([1, 1, 0, 1, 1, 1, 0], bool)) == 3 and longest_run(np.zeros(4, bool)) == 0 and longest_run(np.ones(5, bool)) == 5


# =====================================================================================================================================
# Mel-bank helpers
# =====================================================================================================================================

BANKS = ("whisper80", "htk128", "tel23", "dense24")
BANK_FFT = {"whisper80": 400, "htk128": 512, "tel23": 256, "dense24": 400}
DENSE_EMPTY_ROW = 7
FRAMES = (1, 3, 1031)                        # frames * n_mels is no multiple of 256 for any of the banks


@functools.lru_cache(maxsize=None)
def bank_filters(name):
    """the dense f64 matrix behind each bank (from_mel banks: mel() of the same arguments, tests/test_gpu_parity.py pins the equality)"""
    O = _oracle()
    if name == "whisper80":
        return O.mel_filterbank(16000.0, 400, 80)
    if name == "htk128":
        return O.mel_filterbank(16000.0, 512, 128, 20.0, None, True, True)
    if name == "tel23":
        return O.mel_filterbank(8000.0, 256, 23, None, 3800.0, False, False)
    fb = np.array(O.mel_filterbank(16000.0, 400, 24), np.float64)            # dense: one all-zero row, one negative weight
    fb[DENSE_EMPTY_ROW] = 0.0
    nz = np.flatnonzero(fb[12])
    assert nz.size >= 5
    k = nz[int(np.argmin(fb[12, nz]))]
    fb[12, k] = -fb[12, k]
    return fb


def make_bank(gpu, name):
    if name == "whisper80":
        return gpu.SparseMelFilterbank.from_mel(16000.0, 400, 80)
    if name == "htk128":
        return gpu.SparseMelFilterbank.from_mel(16000.0, 512, 128, f_min=20.0, htk=True)
    if name == "tel23":
        return gpu.SparseMelFilterbank.from_mel(8000.0, 256, 23, f_max=3800.0, norm=False)
    return gpu.SparseMelFilterbank.from_dense(bank_filters(name))


@functools.lru_cache(maxsize=None)
def power_case(name, n_frames, f64):
    O = _oracle()
    fb = bank_filters(name)
    T = np.float64 if f64 else np.float32
    p = (np.random.default_rng(100 + n_frames + fb.shape[0]).standard_normal((n_frames, fb.shape[1])) ** 2).astype(T)
    return p, O.project_power(fb, p)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BANKS)
def test_gpu_bank_project_power_device(gpu, name):
    """melspec_bank_project_power_device, f32 and f64, 1 / 3 / 1031 frames (the last block is partial): bit for bit against
    project_power; a row without weights gives +0.0; a negative weight is summed like any other."""
    bank = make_bank(gpu, name)
    nm, bins = bank.n_mels, bank.fft_bins
    assert (nm, bins) == bank_filters(name).shape
    for f64 in (False, True):
        for nf in FRAMES:
            assert (nf * nm) % 256 != 0
            p, want = power_case(name, nf, f64)
            d = _upload(gpu, p)
            for label, stream in _streams():
                what = f"project_power {name} {'f64' if f64 else 'f32'} {nf} frames ({label})"
                out = Fence(gpu, nf * nm * (2 if f64 else 1))
                bank.project_power_device(d.ptr, p.dtype, nf, out.ptr, stream=_sp(stream))
                gpu.device_synchronize()
                got = check_words(out, [(0, _u32(want))], what)[0]
                if name == "dense24":
                    assert not got.view(want.dtype).reshape(nf, nm)[:, DENSE_EMPTY_ROW].view(np.uint32 if not f64 else np.uint64).any(), "the empty row is +0.0"
            d.free()
    bank.close()


@functools.lru_cache(maxsize=None)
def log_mel_case(name):
    """(the 1031 full-width frames of compute_all_cpu on synthetic PCM, the oracle's log-mel of them)"""
    O = _oracle()
    n_fft = BANK_FFT[name]
    hop = n_fft // 4
    spec = O.compute_all_cpu(O.synth_pcm(17, n_fft + 1030 * hop), n_fft, hop)
    assert spec.shape == (1031, n_fft)
    return spec, O.log_mel_spectrogram(spec, bank_filters(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BANKS)
def test_gpu_bank_log_mel_device(gpu, name):
    """melspec_bank_log_mel_device on the full n_fft bins of compute_all_cpu, complex128 within 1e-12 and complex64 within 1e-5 of
    log_mel_spectrogram (the tolerances of test_sparse_filterbank_helpers), 1 and 1031 frames; the Nyquist bin contributes nothing:
    another value there gives the same bits; n_fft < fft_bins is refused with nothing written."""
    bank = make_bank(gpu, name)
    nm, n_fft = bank.n_mels, BANK_FFT[name]
    spec, want = log_mel_case(name)
    other = spec.copy()
    other[:, n_fft // 2] += 1000.0 - 500.0j
    for dt, tol in ((np.complex128, 1e-12), (np.complex64, 1e-5)):
        for nf in (1, 1031):
            d, d2 = _upload(gpu, spec[:nf].astype(dt)), _upload(gpu, other[:nf].astype(dt))
            for label, stream in _streams():
                what = f"log_mel {name} {np.dtype(dt).name} {nf} frames ({label})"
                out, out2 = Fence(gpu, nf * nm * 2), Fence(gpu, nf * nm * 2)
                bank.log_mel_device(d.ptr, dt, n_fft, nf, out.ptr, stream=_sp(stream))
                bank.log_mel_device(d2.ptr, dt, n_fft, nf, out2.ptr, stream=_sp(stream))
                gpu.device_synchronize()
                got = check_doubles(out, [(0, want[:nf])], what, tol=tol)[0]
                got2 = check_doubles(out2, [(0, want[:nf])], what + ", another Nyquist bin", tol=tol)[0]
                assert np.array_equal(got, got2), what + ": the Nyquist bin changed the result"
            d.free(); d2.free()
    d = _upload(gpu, spec[:3])
    for label, stream in _streams():
        out = Fence(gpu, 3 * nm * 2)
        with pytest.raises(gpu.HipRuntimeError):
            bank.log_mel_device(d.ptr, np.complex128, bank.fft_bins - 1, 3, out.ptr, stream=_sp(stream))
        gpu.device_synchronize()
        check_doubles(out, [], f"log_mel {name}: n_fft < fft_bins ({label})")
    d.free(); bank.close()


def norm_input(n, f64, kind):
    """log-mel-like values in (-12, 0): with the maximum 0.5 about a third of them fall under mmax - 8"""
    T = np.float64 if f64 else np.float32
    x = np.random.default_rng(300 + n % 1000 + len(kind)).uniform(-12.0, 0.0, n).astype(T)
    if kind == "max-last":
        x[n - 1] = 0.5
    elif kind == "max-first":
        x[0] = 0.5
    elif kind == "nan":
        x[:] = np.nan
    elif kind == "equal":
        x[:] = -3.25
    if kind in ("max-last", "max-first") and n > 1000:
        x[np.random.default_rng(5).integers(1, n - 1, n // 997)] = np.nan          # NaNs sprinkled through
        x[n // 2], x[n // 2 + 1] = -0.0, 0.0
    return x


def _norm_call(gpu, bank, x, stream, what):
    O = _oracle()
    f64 = x.dtype == np.float64
    with np.errstate(invalid="ignore"):
        want = O.norm_mel(x)
    assert want.dtype == x.dtype
    d = _upload(gpu, x)
    out = Fence(gpu, x.size * (2 if f64 else 1))
    bank.norm_mel_device(d.ptr, x.dtype, x.size, out.ptr, stream=_sp(stream))
    gpu.device_synchronize()
    check_words(out, [(0, _u32(want))], what)
    d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [False, True])
def test_gpu_bank_norm_mel_device(gpu, f64):
    """melspec_bank_norm_mel_device bit for bit against norm_mel: 1, 255, 257 values and 2 * cus * 4096 + 257 (norm_launch caps the grid
    at cus * 16 blocks of 256: the tail sits in the third grid-stride pass) with the maximum at the last index, then at the first, NaNs
    sprinkled through and a -0.0 / +0.0 pair; all-NaN and all-equal inputs."""
    bank = make_bank(gpu, "whisper80")
    big = 2 * _cus() * 4096 + 257
    for label, stream in _streams():
        for n in (1, 255, 257):
            _norm_call(gpu, bank, norm_input(n, f64, "max-last"), stream, f"norm_mel {n} values ({label})")
        for kind in ("max-last", "max-first"):
            _norm_call(gpu, bank, norm_input(big, f64, kind), stream, f"norm_mel {big} values, {kind} ({label})")
        for kind in ("nan", "equal"):
            _norm_call(gpu, bank, norm_input(257, f64, kind), stream, f"norm_mel 257 values, {kind} ({label})")
    bank.close()


@pytest.mark.gpu
def test_gpu_bank_norm_mel_two_caller_streams(gpu):
    """Two calls back to back on two caller streams with different inputs and maxima, each synchronised on its own stream: the bank's
    one scratch word is handed from the first stream to the second (key_used / key_stream), both results are right."""
    O = _oracle()
    bank = make_bank(gpu, "tel23")
    big = 2 * _cus() * 4096 + 257
    a, b = norm_input(big, False, "max-last"), norm_input(4099, False, "max-first") - np.float32(20.0)
    da, db = _upload(gpu, a), _upload(gpu, b)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for first, second in ((s1, s2), (s2, s1)):
        fa, fb = Fence(gpu, a.size), Fence(gpu, b.size)
        gpu.device_synchronize()
        bank.norm_mel_device(da.ptr, a.dtype, a.size, fa.ptr, stream=first.cuda_stream)
        bank.norm_mel_device(db.ptr, b.dtype, b.size, fb.ptr, stream=second.cuda_stream)
        first.synchronize()
        second.synchronize()
        check_words(fa, [(0, _u32(O.norm_mel(a)))], "norm_mel on the first caller stream")
        check_words(fb, [(0, _u32(O.norm_mel(b)))], "norm_mel on the second caller stream")
    da.free(); db.free(); bank.close()
