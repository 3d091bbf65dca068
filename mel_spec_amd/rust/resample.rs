//! `src/hip_resample.rs` for wavey-ai/mel-spec -- the resampler in front of the MI355X (gfx950) frontends, behind feature `hip`.
//!
//! NOT COMPILED IN THIS REPOSITORY (the build image has no Rust toolchain).  Thin: all work happens behind the C ABI of
//! `libmelspec_hip.so` (include/melspec_resample.h: the definition of the filter, the conventions, the statuses).  A file of its own:
//! the externs of `hip.rs` are those of include/melspec_hip.h.
use std::ffi::{c_char, c_int, c_void, CStr};

use crate::hip::HipError;

pub const PCM_F32: c_int = 0;
pub const PCM_S16: c_int = 1;

#[repr(C)]
struct Handle {
    _private: [u8; 0],
}

#[link(name = "melspec_hip")]
unsafe extern "C" {
    fn melspec_last_error() -> *const c_char;
    fn melspec_resample_geometry(rate_in: u32, rate_out: u32, orig: *mut u32, new_rate: *mut u32, width: *mut u32, max_inside_taps: *mut u32) -> c_int;
    fn melspec_resample_taps(rate_in: u32, rate_out: u32, taps: *mut f64, capacity: usize) -> c_int;
    fn melspec_resample_out_len(rate_in: u32, rate_out: u32, n_in: usize) -> usize;
    fn melspec_resampler_create(out: *mut *mut Handle, device: c_int, rate_in: u32, rate_out: u32) -> c_int;
    fn melspec_resampler_destroy(r: *mut Handle);
    fn melspec_resampler_kernel_name(r: *const Handle) -> *const c_char;
    fn melspec_resample_uniform_device(r: *mut Handle, d_pcm: *const c_void, pcm_dtype: c_int, clip_stride: u64, clip_len: u64, n_clips: u32,
                                       d_out: *mut f32, out_stride: u64, stream: *mut c_void) -> c_int;
    fn melspec_resample_ragged_device(r: *mut Handle, d_pcm: *const c_void, pcm_dtype: c_int, h_offsets: *const u64, h_lengths: *const u64, n_clips: u32,
                                      d_out: *mut f32, h_out_offsets: *const u64, stream: *mut c_void) -> c_int;
    fn melspec_resample_host(r: *mut Handle, samples: *const c_void, pcm_dtype: c_int, n_samples: usize, out: *mut f32, out_capacity: usize,
                             n_out: *mut usize) -> c_int;
    fn melspec_resampler_synchronize(r: *mut Handle, stream: *mut c_void) -> c_int;
}

fn runtime(rc: c_int) -> Result<(), HipError> {
    if rc == 0 {
        return Ok(());
    }
    let m = unsafe { melspec_last_error() };
    let text = if m.is_null() { String::new() } else { unsafe { CStr::from_ptr(m) }.to_string_lossy().into_owned() };
    Err(HipError::Runtime(format!("[{rc}] {text}")))
}

/// orig, new, width, max_inside_taps of a rate pair; K = 2 * width + orig.
#[derive(Debug, Clone, Copy, Default, PartialEq, Eq)]
pub struct Geometry {
    pub orig: u32,
    pub new_rate: u32,
    pub width: u32,
    pub max_inside_taps: u32,
}

pub fn geometry(rate_in: u32, rate_out: u32) -> Result<Geometry, HipError> {
    let mut g = Geometry::default();
    runtime(unsafe { melspec_resample_geometry(rate_in, rate_out, &mut g.orig, &mut g.new_rate, &mut g.width, &mut g.max_inside_taps) })?;
    Ok(g)
}

/// The dense tap table, `[new][K]` row-major.
pub fn taps(rate_in: u32, rate_out: u32) -> Result<Vec<f64>, HipError> {
    let g = geometry(rate_in, rate_out)?;
    let mut h = vec![0f64; g.new_rate as usize * (2 * g.width + g.orig) as usize];
    runtime(unsafe { melspec_resample_taps(rate_in, rate_out, h.as_mut_ptr(), h.len()) })?;
    Ok(h)
}

pub struct HipResampler {
    r: *mut Handle,
    rate_in: u32,
    rate_out: u32,
}

// one resampler per thread and device, like `&mut self`
unsafe impl Send for HipResampler {}

impl HipResampler {
    pub fn new(rate_in: u32, rate_out: u32) -> Result<Self, HipError> {
        let mut r: *mut Handle = std::ptr::null_mut();
        match unsafe { melspec_resampler_create(&mut r, -1, rate_in, rate_out) } {
            0 => Ok(Self { r, rate_in, rate_out }),
            -1 => Err(HipError::Unavailable("rate_in and rate_out must be non-zero")),
            -2 => Err(HipError::Unavailable("no gfx950 (MI355X) device visible to the HIP runtime")),
            -4 => Err(HipError::Unavailable("rate_in / gcd or rate_out / gcd is above 4096")),
            _ => Err(HipError::Unavailable("HIP resampler failed to initialise")),
        }
    }

    pub fn out_len(&self, n_in: usize) -> usize {
        unsafe { melspec_resample_out_len(self.rate_in, self.rate_out, n_in) }
    }

    pub fn kernel_name(&self) -> String {
        unsafe { CStr::from_ptr(melspec_resampler_kernel_name(self.r)) }.to_string_lossy().into_owned()
    }

    /// One clip of f32 samples, host memory in and out.
    pub fn resample(&mut self, samples: &[f32]) -> Result<Vec<f32>, HipError> {
        self.host(samples.as_ptr().cast(), PCM_F32, samples.len())
    }

    /// One clip of int16 samples (value `s * 2^-15`), host memory in and out.
    pub fn resample_i16(&mut self, samples: &[i16]) -> Result<Vec<f32>, HipError> {
        self.host(samples.as_ptr().cast(), PCM_S16, samples.len())
    }

    fn host(&mut self, samples: *const c_void, pcm_dtype: c_int, n: usize) -> Result<Vec<f32>, HipError> {
        let mut out = vec![0f32; self.out_len(n)];
        let mut n_out = 0usize;
        runtime(unsafe { melspec_resample_host(self.r, samples, pcm_dtype, n, out.as_mut_ptr(), out.len(), &mut n_out) })?;
        out.truncate(n_out);
        Ok(out)
    }

    /// Device memory in, device memory out; stream-ordered and asynchronous.
    ///
    /// # Safety
    /// `d_pcm` / `d_out` are device pointers that cover the batch; `stream` is a `hipStream_t` or null (the resampler's own).
    pub unsafe fn uniform_device(&mut self, d_pcm: *const c_void, pcm_dtype: c_int, clip_stride: u64, clip_len: u64, n_clips: u32, d_out: *mut f32,
                                 out_stride: u64, stream: *mut c_void) -> Result<(), HipError> {
        runtime(unsafe { melspec_resample_uniform_device(self.r, d_pcm, pcm_dtype, clip_stride, clip_len, n_clips, d_out, out_stride, stream) })
    }

    /// # Safety
    /// As `uniform_device`; `out_offsets == None`: packed in clip order.
    pub unsafe fn ragged_device(&mut self, d_pcm: *const c_void, pcm_dtype: c_int, offsets: &[u64], lengths: &[u64], d_out: *mut f32,
                                out_offsets: Option<&[u64]>, stream: *mut c_void) -> Result<(), HipError> {
        assert!(offsets.len() == lengths.len() && out_offsets.map_or(true, |o| o.len() == offsets.len()));
        let oo = out_offsets.map_or(std::ptr::null(), |o| o.as_ptr());
        runtime(unsafe { melspec_resample_ragged_device(self.r, d_pcm, pcm_dtype, offsets.as_ptr(), lengths.as_ptr(), offsets.len() as u32, d_out, oo, stream) })
    }

    pub fn synchronize(&mut self, stream: *mut c_void) -> Result<(), HipError> {
        runtime(unsafe { melspec_resampler_synchronize(self.r, stream) })
    }
}

impl Drop for HipResampler {
    fn drop(&mut self) {
        unsafe { melspec_resampler_destroy(self.r) }
    }
}
