//! mi355x.rs -- glue between halo2_proofs::arithmetic and libhalo2_mi355x.so (added by rust/halo2_proofs.patch).
//! Maintained by hand (not generated: the sys:: items it uses are checked against the header
//! by the repository's tests).  The two functions return None / false whenever the GPU path does not apply or fails
//! WITHOUT having touched the caller's arrays, and the caller falls through to the untouched upstream body: other
//! curves / fields, tiny inputs, no device, any error code but HM_ERR_PARTIAL_OUTPUT (which panics: see try_best_fft).
//! Needs nothing newer than Rust 1.56: std::sync::Once + AtomicBool for the one-time check (the pinned tag predates the 1.70 cell types).
// halo2_proofs' lib.rs denies these crate-wide (as recalled: #![deny(missing_docs)], #![deny(missing_debug_implementations)],
// #![deny(unsafe_code)]); this module is FFI glue -- the allowance is scoped to it.
#![allow(unsafe_code, missing_docs, missing_debug_implementations, clippy::all)]
use std::any::TypeId;
use std::sync::atomic::{AtomicBool, Ordering};
use std::sync::Once;

use group::prime::PrimeCurveAffine; // G1Affine::generator()
use group::Group as _; // G1::identity()
use halo2_mi355x_sys as sys;
use halo2curves::bn256::{Fr, G1Affine, G1};
use halo2curves::CurveAffine;

use crate::arithmetic::Group;

/// Below these sizes the host-pointer round trip (launch + PCIe latency) is no faster than the CPU body: measured
/// crossover against a 16-core host, stay on the CPU.
// MEASURED (tools/crossover.py on the MI355X box against oracle/cpu_ref.c on its 16 granted cores; table in DESIGN.md
// section 8 and profiles/r04_crossover.json).  MSM: 0.30 ms against 1.4 ms (16 threads) / 5.4 ms (1 thread) at 2^8, the
// smallest size measured.  NTT: 0.057 ms against 0.111 ms on one thread at 2^10; 2^9 is a tie, 2^8 loses.
// bench.py reads both values from the two lines below: keep their spelling.
pub const GPU_MIN_LOG_N_MSM: u32 = 8;
pub const GPU_MIN_LOG_N_NTT: u32 = 10;
/// best_fft over G1 (g_to_lagrange, ParamsKZG::downsize): every butterfly is a 254-bit scalar multiplication, so the GPU wins
/// far earlier than for Fr.  ESTIMATE, not a measurement: no Rust toolchain has timed the CPU body against hm_g1_fft_bn256
/// yet; re-measure the crossover when one does.
pub const GPU_MIN_LOG_N_G1_FFT: u32 = 6;

fn layout_check() -> bool {
    if std::mem::size_of::<Fr>() != 32 || std::mem::size_of::<G1Affine>() != 64 || std::mem::size_of::<G1>() != 96 {
        return false;
    }
    // the generator (1, 2) must read back as x = R mod p, y = 2R mod p (Montgomery words, x before y)
    let g: [u64; 8] = unsafe { std::mem::transmute(<G1Affine as PrimeCurveAffine>::generator()) };
    g[..4] == [0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f]
        && g[4..] == [0xa6ba871b8b1e1b3a, 0x14f1d651eb8e167b, 0xccdd46def0f28c58, 0x1c14ef83340fbe5e]
        && unsafe { sys::hm_device_count() } > 0
}

/// halo2curves gives these types no #[repr(C)]; the byte layout the library reads is asserted instead (once).
pub fn layout_ok() -> bool {
    static INIT: Once = Once::new();
    static OK: AtomicBool = AtomicBool::new(false);
    INIT.call_once(|| OK.store(layout_check(), Ordering::Release));
    OK.load(Ordering::Acquire)
}

/// (x, y, 1) Montgomery words, or all zero for the identity: exactly bn256::G1 { x, y, z }.
pub fn g1_from_words(xyz: [u64; 12]) -> G1 {
    if xyz[8..].iter().all(|w| *w == 0) {
        <G1 as group::Group>::identity()
    } else {
        unsafe { std::mem::transmute::<[u64; 12], G1>(xyz) }
    }
}

pub fn try_best_multiexp<C: CurveAffine>(coeffs: &[C::Scalar], bases: &[C]) -> Option<C::Curve> {
    if TypeId::of::<C>() != TypeId::of::<G1Affine>() || coeffs.len() < (1 << GPU_MIN_LOG_N_MSM) || !layout_ok() {
        return None;
    }
    let mut xyz = [0u64; 12];
    let rc = unsafe {
        sys::hm_msm_bn256_g1_jacobian(coeffs.as_ptr() as *const u64, bases.as_ptr() as *const u64, coeffs.len(), xyz.as_mut_ptr())
    };
    if rc != sys::HM_OK {
        return None; // error policy of the boundary: fall back to the CPU body (the inputs are untouched)
    }
    let p = g1_from_words(xyz);
    Some(unsafe { std::mem::transmute_copy::<G1, C::Curve>(&p) }) // C::Curve == G1 here (checked by the TypeId test above)
}

pub fn try_best_fft<G: Group>(a: &mut [G], omega: &G::Scalar, log_n: u32) -> bool {
    if TypeId::of::<G>() == TypeId::of::<G1>() {
        return try_best_fft_g1(a, omega, log_n);
    }
    if TypeId::of::<G>() != TypeId::of::<Fr>() || log_n < GPU_MIN_LOG_N_NTT || log_n > 28 || !layout_ok() {
        return false;
    }
    let rc = unsafe { sys::hm_ntt_bn256_fr(a.as_mut_ptr() as *mut u64, omega as *const _ as *const u64, log_n) };
    if rc == sys::HM_ERR_PARTIAL_OUTPUT {
        // the copy of the result back into `a` failed half-way: `a` is neither the input nor the output any more, so the
        // CPU body must NOT run on it (it would continue the proof with a silently wrong polynomial)
        panic!("hm_ntt_bn256_fr: {}", sys::last_error());
    }
    rc == sys::HM_OK // every other error code leaves `a` exactly as it was: the caller runs the CPU body
}

/// best_fft::<G1> (upstream's g_to_lagrange calls it with omega^-1 and scales afterwards): hm_g1_fft_bn256 on the Jacobian array
/// in place, outputs normalised to (x, y, 1) with the identity mapped through g1_from_words to G1::identity().
fn try_best_fft_g1<G: Group>(a: &mut [G], omega: &G::Scalar, log_n: u32) -> bool {
    if TypeId::of::<G::Scalar>() != TypeId::of::<Fr>() || log_n < GPU_MIN_LOG_N_G1_FFT || log_n > 24 || !layout_ok() {
        return false;
    }
    let rc = unsafe { sys::hm_g1_fft_bn256(a.as_mut_ptr() as *mut u64, omega as *const _ as *const u64, log_n, std::ptr::null()) };
    if rc == sys::HM_ERR_PARTIAL_OUTPUT {
        // as in the Fr branch: `a` is neither the input nor the output any more, the CPU body must not run on it
        panic!("hm_g1_fft_bn256: {}", sys::last_error());
    }
    if rc != sys::HM_OK {
        return false; // `a` untouched: the caller runs the CPU body
    }
    for p in a.iter_mut() {
        // G == G1 here (TypeId-checked above; 96 bytes by layout_ok): identities come back as all-zero words
        let xyz = unsafe { std::mem::transmute_copy::<G, [u64; 12]>(p) };
        let q = g1_from_words(xyz);
        *p = unsafe { std::mem::transmute_copy::<G1, G>(&q) };
    }
    true
}

/// R mod r: bn256::Fr::one() as the four Montgomery words the library reads (spelled out: no dependence on the ff version's `one()` / `ONE`).
pub(crate) const FR_ONE: [u64; 4] = [0xac96341c4ffffffb, 0x36fc76959f60cd29, 0x666ea36f7879462e, 0x0e0a77c19a07df2f];

/// The same as an `Fr` (Montgomery words are the in-memory form: layout_ok() has checked 32 bytes).
#[allow(dead_code)]
pub(crate) fn fr_one() -> Fr {
    unsafe { std::mem::transmute_copy::<[u64; 4], Fr>(&FR_ONE) }
}

fn fr_words<S>(s: &S) -> [u64; 4] {
    unsafe { std::mem::transmute_copy::<S, [u64; 4]>(s) } // S == Fr here (TypeId-checked by the callers; 32 bytes by layout_ok)
}

/// EvaluationDomain::coeff_to_extended in one library call (hm_coeff_to_extended_bn256_fr): `a` holds the 2^k coefficients on
/// entry and, when this returns true, the 2^extended_k evaluations on the zeta-coset.  Only the 2^k coefficients cross PCIe
/// upwards (never the zero padding `resize` would append); distribute_powers_zeta is fused into the first NTT pass.  The result
/// is written to a FRESH Vec that replaces `a` only on success, so every failure -- HM_ERR_PARTIAL_OUTPUT included -- leaves
/// `a` exactly as it was and the caller runs the CPU body.  (The fresh allocation's first-touch page faults replace the ones upstream's own
/// `resize` to the extended length takes; the library touches the pages from helper threads while the transform runs.)
pub fn try_coeff_to_extended<G: Group>(a: &mut Vec<G>, extended_omega: &G::Scalar, k: u32, extended_k: u32, g_coset: &G::Scalar,
                                       g_coset_inv: &G::Scalar) -> bool {
    if TypeId::of::<G>() != TypeId::of::<Fr>() || TypeId::of::<G::Scalar>() != TypeId::of::<Fr>() || extended_k < GPU_MIN_LOG_N_NTT
        || extended_k > 28 || k > extended_k || a.len() != (1usize << k) || !layout_ok()
    {
        return false;
    }
    // a[i] *= [1, g_coset, g_coset_inv][i % 3]: distribute_powers_zeta(a, true) (zeta^3 = 1, so g_coset_inv = zeta^2)
    let mut coset = [0u64; 12];
    coset[..4].copy_from_slice(&FR_ONE);
    coset[4..8].copy_from_slice(&fr_words(g_coset));
    coset[8..].copy_from_slice(&fr_words(g_coset_inv));
    let len = 1usize << extended_k;
    let mut ext: Vec<G> = Vec::with_capacity(len);
    let rc = unsafe {
        sys::hm_coeff_to_extended_bn256_fr(a.as_ptr() as *const u64, ext.as_mut_ptr() as *mut u64, extended_omega as *const _ as *const u64,
                                           k, extended_k, coset.as_ptr())
    };
    if rc != sys::HM_OK {
        return false; // `ext` (possibly half-written) is dropped; `a` is untouched
    }
    unsafe { ext.set_len(len) }; // every element was written by the library's final copy
    *a = ext;
    true
}

/// EvaluationDomain::extended_to_coeff in one library call (hm_extended_to_coeff_bn256_fr): in place on the 2^extended_k
/// evaluations; the ifft divisor and distribute_powers_zeta(a, false) ride on the last NTT pass, only the `keep` coefficients
/// upstream keeps come back over PCIe, and `a` is truncated to them.
pub fn try_extended_to_coeff<G: Group>(a: &mut Vec<G>, extended_omega_inv: &G::Scalar, extended_k: u32, divisor: &G::Scalar,
                                       g_coset: &G::Scalar, g_coset_inv: &G::Scalar, keep: usize) -> bool {
    if TypeId::of::<G>() != TypeId::of::<Fr>() || TypeId::of::<G::Scalar>() != TypeId::of::<Fr>() || extended_k < GPU_MIN_LOG_N_NTT
        || extended_k > 28 || a.len() != (1usize << extended_k) || keep > a.len() || !layout_ok()
    {
        return false;
    }
    // a[i] *= [1, g_coset_inv, g_coset][i % 3]: distribute_powers_zeta(a, false)
    let mut coset_inv = [0u64; 12];
    coset_inv[..4].copy_from_slice(&FR_ONE);
    coset_inv[4..8].copy_from_slice(&fr_words(g_coset_inv));
    coset_inv[8..].copy_from_slice(&fr_words(g_coset));
    let rc = unsafe {
        sys::hm_extended_to_coeff_bn256_fr(a.as_mut_ptr() as *mut u64, keep, extended_omega_inv as *const _ as *const u64, extended_k,
                                           divisor as *const _ as *const u64, coset_inv.as_ptr())
    };
    if rc == sys::HM_ERR_PARTIAL_OUTPUT {
        panic!("hm_extended_to_coeff_bn256_fr: {}", sys::last_error()); // as in try_best_fft: `a` is neither input nor output
    }
    if rc != sys::HM_OK {
        return false;
    }
    a.truncate(keep);
    true
}

/// One process, several GPUs: every later best_multiexp / registered base set is split over `devices` inside the library.
pub fn use_devices(devices: &[i32]) -> bool {
    unsafe { sys::hm_set_msm_devices(devices.as_ptr(), devices.len() as i32) == sys::HM_OK }
}
