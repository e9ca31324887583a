//! mi355x_kzg.rs -- ParamsKZG's side of the binding (added by rust/halo2_proofs.patch / rust/apply_edits.py next to
//! mi355x.rs, declared in arithmetic.rs).  Maintained by hand.
//!
//! create_proof commits ~56 times per MerkleSumTree proof (/root/reference/src/circuits/utils.rs:40-48), always against
//! the same two arrays, params.g and params.g_lagrange.  The free-function drop-in (mi355x.rs) re-reads the whole base
//! array on every call to key its cache; here every ParamsKZG registers its two arrays ONCE (hm_register_bases: converted,
//! resident in HBM, from 2^17 points with the fixed-base table) and commits through the handle, and a whole phase of
//! commitments goes to the library in one call (hm_msm_batch_bn256_g1_h: eight in flight, uploads behind kernels).
//!
//! `SrsHandles` is a FIELD of ParamsKZG (`gpu`), so a handle can never outlive or alias the arrays it was made from:
//! every constructor creates it empty (Default), Clone creates a fresh empty one (the clone owns new Vecs), Drop releases
//! both sets, and a handle is used only while the Vec it came from still starts at the same address and is at least as
//! long as when it was registered (`downsize` truncates g in place -- a prefix, still valid -- and REPLACES g_lagrange,
//! whose new buffer fails that test and is registered afresh).
// halo2_proofs' lib.rs denies these crate-wide (as recalled: #![deny(missing_docs)], #![deny(missing_debug_implementations)],
// #![deny(unsafe_code)]); this module is FFI glue -- the allowance is scoped to it.
#![allow(unsafe_code, missing_docs, missing_debug_implementations, clippy::all)]
use std::any::TypeId;
use std::fmt;
use std::sync::atomic::{AtomicU64, AtomicUsize, Ordering};
use std::sync::Mutex;

use halo2_mi355x_sys as sys;
use halo2curves::bn256::{G1Affine, G1};
use halo2curves::CurveAffine;

use crate::arithmetic::mi355x::{g1_from_words, layout_ok, GPU_MIN_LOG_N_MSM};

const UNSET: u64 = 0; // the library's handles start at 1
const FAILED: u64 = u64::MAX; // registration failed once: do not try again for this array

struct Slot {
    handle: AtomicU64,
    ptr: AtomicUsize,
    len: AtomicUsize,
}

impl Slot {
    const fn new() -> Self {
        Slot { handle: AtomicU64::new(UNSET), ptr: AtomicUsize::new(0), len: AtomicUsize::new(0) }
    }
    fn release(&self) {
        let h = self.handle.swap(UNSET, Ordering::AcqRel);
        if h != UNSET && h != FAILED {
            unsafe { sys::hm_release_bases(h) };
        }
    }
}

pub struct SrsHandles {
    g: Slot,
    g_lagrange: Slot,
    lock: Mutex<()>, // registration happens once per array, under this lock
}

impl Default for SrsHandles {
    fn default() -> Self {
        SrsHandles { g: Slot::new(), g_lagrange: Slot::new(), lock: Mutex::new(()) }
    }
}
impl Clone for SrsHandles {
    fn clone(&self) -> Self {
        Self::default() // the clone of a ParamsKZG owns new Vecs: it registers them itself on first use
    }
}
impl fmt::Debug for SrsHandles {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        write!(f, "SrsHandles {{ g: {}, g_lagrange: {} }}", self.g.handle.load(Ordering::Relaxed), self.g_lagrange.handle.load(Ordering::Relaxed))
    }
}
impl Drop for SrsHandles {
    fn drop(&mut self) {
        self.g.release();
        self.g_lagrange.release();
    }
}

impl SrsHandles {
    /// Drop both device sets (ParamsKZG::downsize replaces g_lagrange and shortens g): registered afresh on demand.
    pub fn reset(&self) {
        let _turn = self.lock.lock().unwrap_or_else(|e| e.into_inner());
        self.g.release();
        self.g_lagrange.release();
    }

    /// The handle of `bases` (registering it on first use), or None: not bn256, too small, no device, registration failed.
    fn handle_for(&self, slot: &Slot, bases: &[G1Affine], n: usize) -> Option<u64> {
        if n < (1 << GPU_MIN_LOG_N_MSM) || n > bases.len() || !layout_ok() {
            return None;
        }
        let same_array = |s: &Slot| s.ptr.load(Ordering::Acquire) == bases.as_ptr() as usize && s.len.load(Ordering::Acquire) >= n;
        let h = slot.handle.load(Ordering::Acquire);
        if h != UNSET && same_array(slot) {
            return if h == FAILED { None } else { Some(h) };
        }
        let _turn = self.lock.lock().unwrap_or_else(|e| e.into_inner());
        let h = slot.handle.load(Ordering::Acquire);
        if h != UNSET && same_array(slot) {
            return if h == FAILED { None } else { Some(h) };
        }
        slot.release(); // another array (downsize replaced it): the old set goes
        let mut out = 0u64;
        let rc = unsafe { sys::hm_register_bases(bases.as_ptr() as *const u64, bases.len(), &mut out) };
        slot.ptr.store(bases.as_ptr() as usize, Ordering::Release);
        slot.len.store(bases.len(), Ordering::Release);
        slot.handle.store(if rc == sys::HM_OK { out } else { FAILED }, Ordering::Release);
        if rc == sys::HM_OK { Some(out) } else { None }
    }

    fn msm<C: CurveAffine>(&self, slot: &Slot, scalars: &[C::Scalar], bases: &[C]) -> Option<C::Curve> {
        if TypeId::of::<C>() != TypeId::of::<G1Affine>() {
            return None;
        }
        let bases: &[G1Affine] = unsafe { std::slice::from_raw_parts(bases.as_ptr() as *const G1Affine, bases.len()) };
        let h = self.handle_for(slot, bases, scalars.len())?;
        let (mut xy, mut is_id) = ([0u64; 8], 0i32);
        let rc = unsafe { sys::hm_msm_bn256_g1_h(h, 0, scalars.as_ptr() as *const u64, scalars.len(), xy.as_mut_ptr(), &mut is_id) };
        if rc != sys::HM_OK {
            return None; // the caller runs best_multiexp (pointer form, then the CPU body)
        }
        let mut xyz = [0u64; 12];
        if is_id == 0 {
            xyz[..8].copy_from_slice(&xy);
            xyz[8..].copy_from_slice(&[0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f]); // z = 1 (R mod p)
        }
        let p: G1 = g1_from_words(xyz);
        Some(unsafe { std::mem::transmute_copy::<G1, C::Curve>(&p) })
    }

    /// ParamsKZG::commit: scalars against g[..scalars.len()].
    pub fn commit<C: CurveAffine>(&self, scalars: &[C::Scalar], g: &[C]) -> Option<C::Curve> {
        self.msm::<C>(&self.g, scalars, g)
    }
    /// ParamsKZG::commit_lagrange: scalars against g_lagrange[..scalars.len()].
    pub fn commit_lagrange<C: CurveAffine>(&self, scalars: &[C::Scalar], g_lagrange: &[C]) -> Option<C::Curve> {
        self.msm::<C>(&self.g_lagrange, scalars, g_lagrange)
    }

    /// The commitments of one prover phase (columns of one length) in ONE library call; None = fall back to one by one.
    pub fn commit_lagrange_batch<C: CurveAffine>(&self, columns: &[&[C::Scalar]], g_lagrange: &[C]) -> Option<Vec<C::Curve>> {
        if TypeId::of::<C>() != TypeId::of::<G1Affine>() || columns.is_empty() {
            return None;
        }
        let n = columns[0].len();
        if columns.iter().any(|c| c.len() != n) {
            return None;
        }
        let bases: &[G1Affine] = unsafe { std::slice::from_raw_parts(g_lagrange.as_ptr() as *const G1Affine, g_lagrange.len()) };
        let h = self.handle_for(&self.g_lagrange, bases, n)?;
        let ptrs: Vec<*const u64> = columns.iter().map(|c| c.as_ptr() as *const u64).collect();
        let mut out = vec![0u64; 12 * columns.len()];
        let rc = unsafe { sys::hm_msm_batch_bn256_g1_h(h, 0, ptrs.as_ptr(), n, columns.len(), out.as_mut_ptr()) };
        if rc != sys::HM_OK {
            return None;
        }
        Some(
            out.chunks_exact(12)
                .map(|w| {
                    let mut xyz = [0u64; 12];
                    xyz.copy_from_slice(w);
                    let p: G1 = g1_from_words(xyz);
                    unsafe { std::mem::transmute_copy::<G1, C::Curve>(&p) }
                })
                .collect(),
        )
    }
}
