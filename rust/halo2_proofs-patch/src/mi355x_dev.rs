//! mi355x_dev.rs -- polynomials that STAY in HBM between the steps of create_proof (added by rust/apply_edits.py next to mi355x.rs,
//! declared in arithmetic.rs).  Maintained by hand.
//!
//! The drop-in edits (mi355x.rs, mi355x_kzg.rs) leave every polynomial in a host Vec, so each best_fft / coeff_to_extended moves its
//! array over PCIe twice: 122-292 ms of the k = 18 proof against 34 ms of device time.  This module is the
//! other half of the boundary as code instead of prose: `DevicePoly` (RAII over hm_device_malloc), `DeviceDomain` (the
//! EvaluationDomain steps on device-resident arrays), `commit_dev` / `commit_batch_dev`, `eval_polynomial_dev`, and
//! `QuotientProgram::quotient_by_cosets` -- evaluate_h + divide_by_vanishing_poly + extended_to_coeff in ONE call from coefficient
//! arrays.  A prover adopts it step by step: upload advice columns once (`DevicePoly::from_slice`), commit from the device, transform
//! on the device, bring back only what the transcript needs.  Nothing here is reached by the drop-in edits; nothing here has met rustc.
//! Every function returns None / false on any error (sys::last_error() has the message) and never panics.
// halo2_proofs' lib.rs denies these crate-wide (as recalled: #![deny(missing_docs)], #![deny(missing_debug_implementations)],
// #![deny(unsafe_code)]); this module is FFI glue -- the allowance is scoped to it.
#![allow(unsafe_code, missing_docs, missing_debug_implementations, clippy::all)]
use std::os::raw::c_void;
use std::ptr;

use ff::Field;
use halo2_mi355x_sys as sys;
use halo2curves::bn256::{Fr, G1};

use crate::arithmetic::mi355x::{fr_one, g1_from_words, layout_ok, FR_ONE};

fn words(x: &Fr) -> [u64; 4] {
    unsafe { std::mem::transmute_copy::<Fr, [u64; 4]>(x) } // 32 bytes, Montgomery words (layout_ok() asserts the layout once)
}

/// `len` field elements in device memory; freed on drop (hipFree waits for the device: keep buffers for the life of a proof).
#[derive(Debug)]
pub struct DevicePoly {
    ptr: *mut c_void,
    len: usize,
}
unsafe impl Send for DevicePoly {}

impl DevicePoly {
    pub fn new(len: usize) -> Option<Self> {
        if !layout_ok() {
            return None;
        }
        let mut p: *mut c_void = ptr::null_mut();
        if unsafe { sys::hm_device_malloc(len * 32, &mut p) } != sys::HM_OK {
            return None;
        }
        Some(DevicePoly { ptr: p, len })
    }
    /// Upload (through the library's copy policy, hm_set_host_copies).
    pub fn from_slice(a: &[Fr]) -> Option<Self> {
        let d = Self::new(a.len())?;
        if unsafe { sys::hm_copy_to_device(d.ptr, a.as_ptr() as *const c_void, a.len() * 32) } != sys::HM_OK {
            return None;
        }
        Some(d)
    }
    /// Download after waiting for the device (the steps below are asynchronous on the default stream).
    pub fn to_vec(&self) -> Option<Vec<Fr>> {
        if unsafe { sys::hm_device_synchronize() } != sys::HM_OK {
            return None;
        }
        let mut v: Vec<Fr> = Vec::with_capacity(self.len);
        if unsafe { sys::hm_copy_to_host(v.as_mut_ptr() as *mut c_void, self.ptr as *const c_void, self.len * 32) } != sys::HM_OK {
            return None;
        }
        unsafe { v.set_len(self.len) }; // every element was written by the copy
        Some(v)
    }
    /// Upload `a` to elements [first, first + a.len()) of this array: how a prover fills ONE packed array (the column table of a
    /// `QuotientProgram`, polynomial i at [i n, (i + 1) n)) column by column as synthesis produces them.
    pub fn upload_at(&mut self, first: usize, a: &[Fr]) -> bool {
        if first.checked_add(a.len()).map_or(true, |end| end > self.len) {
            return false;
        }
        let dst = unsafe { (self.ptr as *mut u8).add(first * 32) } as *mut c_void;
        unsafe { sys::hm_copy_to_device(dst, a.as_ptr() as *const c_void, a.len() * 32) == sys::HM_OK }
    }
    /// Upload several arrays in ONE call (hm_copy_many_to_device): `arrays[i]` to elements [firsts[i], firsts[i] + arrays[i].len()).
    /// The copy lanes move them as one transfer: the columns of a proof at the rate of one large array.
    pub fn upload_many_at(&mut self, firsts: &[usize], arrays: &[&[Fr]]) -> bool {
        if firsts.len() != arrays.len() {
            return false;
        }
        let mut dsts: Vec<*mut c_void> = Vec::with_capacity(arrays.len());
        let mut srcs: Vec<*const c_void> = Vec::with_capacity(arrays.len());
        let mut bytes: Vec<usize> = Vec::with_capacity(arrays.len());
        for (&first, a) in firsts.iter().zip(arrays.iter()) {
            if first.checked_add(a.len()).map_or(true, |end| end > self.len) {
                return false;
            }
            dsts.push(unsafe { (self.ptr as *mut u8).add(first * 32) } as *mut c_void);
            srcs.push(a.as_ptr() as *const c_void);
            bytes.push(a.len() * 32);
        }
        unsafe { sys::hm_copy_many_to_device(dsts.as_ptr(), srcs.as_ptr(), bytes.as_ptr(), bytes.len()) == sys::HM_OK }
    }
    /// Download several ranges (first element, length) in ONE call after waiting for the device (hm_copy_many_to_host).
    pub fn to_vecs_ranges(&self, ranges: &[(usize, usize)]) -> Option<Vec<Vec<Fr>>> {
        if ranges.iter().any(|&(first, len)| first.checked_add(len).map_or(true, |end| end > self.len)) || unsafe { sys::hm_device_synchronize() } != sys::HM_OK {
            return None;
        }
        let mut out: Vec<Vec<Fr>> = ranges.iter().map(|&(_, len)| Vec::with_capacity(len)).collect();
        let dsts: Vec<*mut c_void> = out.iter_mut().map(|v| v.as_mut_ptr() as *mut c_void).collect();
        let srcs: Vec<*const c_void> = ranges.iter().map(|&(first, _)| unsafe { (self.ptr as *const u8).add(first * 32) } as *const c_void).collect();
        let bytes: Vec<usize> = ranges.iter().map(|&(_, len)| len * 32).collect();
        if unsafe { sys::hm_copy_many_to_host(dsts.as_ptr(), srcs.as_ptr(), bytes.as_ptr(), bytes.len()) } != sys::HM_OK {
            return None;
        }
        for (v, &(_, len)) in out.iter_mut().zip(ranges.iter()) {
            unsafe { v.set_len(len) }; // every element was written by the copy
        }
        Some(out)
    }
    /// Download elements [first, first + len) after waiting for the device.
    pub fn to_vec_range(&self, first: usize, len: usize) -> Option<Vec<Fr>> {
        if first.checked_add(len).map_or(true, |end| end > self.len) || unsafe { sys::hm_device_synchronize() } != sys::HM_OK {
            return None;
        }
        let src = unsafe { (self.ptr as *const u8).add(first * 32) } as *const c_void;
        let mut v: Vec<Fr> = Vec::with_capacity(len);
        if unsafe { sys::hm_copy_to_host(v.as_mut_ptr() as *mut c_void, src, len * 32) } != sys::HM_OK {
            return None;
        }
        unsafe { v.set_len(len) }; // every element was written by the copy
        Some(v)
    }
    pub fn len(&self) -> usize {
        self.len
    }
    pub fn is_empty(&self) -> bool {
        self.len == 0
    }
    pub fn as_ptr(&self) -> *const c_void {
        self.ptr as *const c_void
    }
    pub fn as_mut_ptr(&mut self) -> *mut c_void {
        self.ptr
    }
}
impl Drop for DevicePoly {
    fn drop(&mut self) {
        if !self.ptr.is_null() {
            unsafe { sys::hm_device_free(self.ptr) };
        }
    }
}

/// The constants of an `EvaluationDomain<Fr>` the device steps need (all of them fields of poly/domain.rs), copied out once.
#[derive(Debug)]
pub struct DeviceDomain {
    pub k: u32,
    pub extended_k: u32,
    pub quotient_poly_degree: usize,
    pub omega: Fr,
    pub omega_inv: Fr,
    pub extended_omega: Fr,
    pub extended_omega_inv: Fr,
    pub g_coset: Fr,
    pub g_coset_inv: Fr,
    pub ifft_divisor: Fr,
    pub extended_ifft_divisor: Fr,
}

impl DeviceDomain {
    pub fn n(&self) -> usize {
        1usize << self.k
    }
    pub fn extended_len(&self) -> usize {
        1usize << self.extended_k
    }
    fn coset_words(&self, scale: Fr) -> [u64; 12] {
        // [1, g_coset, g_coset_inv] * scale: distribute_powers_zeta(a, true) (zeta^3 = 1, so g_coset_inv = zeta^2)
        let mut c = [0u64; 12];
        c[..4].copy_from_slice(&words(&scale));
        c[4..8].copy_from_slice(&words(&(self.g_coset * scale)));
        c[8..].copy_from_slice(&words(&(self.g_coset_inv * scale)));
        c
    }
    /// EvaluationDomain::lagrange_to_coeff on `a.len() / n` back-to-back polynomials, in place: one set of launches.
    pub fn lagrange_to_coeff(&self, a: &mut DevicePoly) -> bool {
        if a.len() == 0 || a.len() % self.n() != 0 {
            return false;
        }
        let (w, d) = (words(&self.omega_inv), words(&self.ifft_divisor));
        unsafe { sys::hm_ntt_batch_bn256_fr_dev(a.as_mut_ptr(), a.len() / self.n(), w.as_ptr(), self.k, d.as_ptr(), ptr::null(), ptr::null_mut()) == sys::HM_OK }
    }
    /// The same on polynomials [first, first + count) of a packed array (polynomial i at [i n, (i + 1) n)).
    pub fn lagrange_to_coeff_range(&self, a: &mut DevicePoly, first: usize, count: usize) -> bool {
        if count == 0 || first.checked_add(count).map_or(true, |end| end * self.n() > a.len()) {
            return false;
        }
        let (w, d) = (words(&self.omega_inv), words(&self.ifft_divisor));
        let p = unsafe { (a.as_mut_ptr() as *mut u8).add(first * self.n() * 32) } as *mut c_void;
        unsafe { sys::hm_ntt_batch_bn256_fr_dev(p, count, w.as_ptr(), self.k, d.as_ptr(), ptr::null(), ptr::null_mut()) == sys::HM_OK }
    }
    /// EvaluationDomain::coeff_to_extended on `a.len() / n` polynomials -> a new array of 2^extended_k evaluations each (the zero
    /// padding is never materialised).  `internal`: the evaluations come out multiplied by 32, the form `QuotientProgram` and
    /// hm_graph_evaluate_flags_dev(HM_GRAPH_COLUMNS_INTERNAL) load without a conversion product.
    pub fn coeff_to_extended(&self, a: &DevicePoly, internal: bool) -> Option<DevicePoly> {
        if a.len() == 0 || a.len() % self.n() != 0 {
            return None;
        }
        let batch = a.len() / self.n();
        let mut ext = DevicePoly::new(batch * self.extended_len())?;
        let coset = self.coset_words(if internal { Fr::from(32u64) } else { fr_one() });
        let w = words(&self.extended_omega);
        let rc = unsafe {
            sys::hm_coeff_to_extended_bn256_fr_dev(a.as_ptr(), ext.as_mut_ptr(), batch, w.as_ptr(), self.k, self.extended_k, coset.as_ptr(), ptr::null_mut())
        };
        if rc == sys::HM_OK { Some(ext) } else { None }
    }
    /// EvaluationDomain::extended_to_coeff in place on `a.len() / 2^extended_k` arrays; the caller reads the first
    /// n * quotient_poly_degree coefficients of each.
    pub fn extended_to_coeff(&self, a: &mut DevicePoly) -> bool {
        if a.len() == 0 || a.len() % self.extended_len() != 0 {
            return false;
        }
        let mut c = [0u64; 12]; // [1, g_coset_inv, g_coset]: distribute_powers_zeta(a, false)
        c[..4].copy_from_slice(&FR_ONE);
        c[4..8].copy_from_slice(&words(&self.g_coset_inv));
        c[8..].copy_from_slice(&words(&self.g_coset));
        let (w, d) = (words(&self.extended_omega_inv), words(&self.extended_ifft_divisor));
        unsafe {
            sys::hm_extended_to_coeff_bn256_fr_dev(a.as_mut_ptr(), a.len() / self.extended_len(), w.as_ptr(), self.extended_k, d.as_ptr(), c.as_ptr(), ptr::null_mut())
                == sys::HM_OK
        }
    }
    /// zeta * extended_omega^j: row E t + j of the extended array is the value at coset_shift(j) * omega^t.
    pub fn coset_shift(&self, j: usize) -> Fr {
        self.g_coset * self.extended_omega.pow_vartime([j as u64])
    }
}

/// ParamsKZG::commit / commit_lagrange with the scalars already on the device (`handle`: hm_register_bases, as SrsHandles keeps it).
pub fn commit_dev(handle: u64, scalars: &DevicePoly) -> Option<G1> {
    let mut xyz = [0u64; 12];
    let rc = unsafe { sys::hm_msm_bn256_g1_dev(handle, 0, scalars.as_ptr(), scalars.len(), ptr::null_mut(), xyz.as_mut_ptr()) };
    if rc != sys::HM_OK {
        return None;
    }
    Some(g1_from_words(xyz))
}

/// A phase of commitments (columns of one length) in one call: eight in flight, dense columns sharing launch chains.
pub fn commit_batch_dev(handle: u64, columns: &[&DevicePoly]) -> Option<Vec<G1>> {
    if columns.is_empty() {
        return Some(Vec::new());
    }
    let n = columns[0].len();
    if columns.iter().any(|c| c.len() != n) {
        return None;
    }
    let ptrs: Vec<*const c_void> = columns.iter().map(|c| c.as_ptr()).collect();
    let mut out = vec![0u64; 12 * columns.len()];
    let rc = unsafe { sys::hm_msm_batch_bn256_g1_dev(handle, 0, ptrs.as_ptr(), n, columns.len(), ptr::null_mut(), out.as_mut_ptr()) };
    if rc != sys::HM_OK {
        return None;
    }
    Some(
        out.chunks_exact(12)
            .map(|w| {
                let mut xyz = [0u64; 12];
                xyz.copy_from_slice(w);
                g1_from_words(xyz)
            })
            .collect(),
    )
}

/// The same for polynomials [first, first + count) of `n` scalars each lying back to back in `polys` (a packed column table, the
/// pieces of h as `QuotientProgram::quotient_by_cosets` returns them): one call, nothing copied.
pub fn commit_pieces_dev(handle: u64, polys: &DevicePoly, n: usize, first: usize, count: usize) -> Option<Vec<G1>> {
    if count == 0 {
        return Some(Vec::new());
    }
    if n == 0 || first.checked_add(count).map_or(true, |end| end.checked_mul(n).map_or(true, |e| e > polys.len())) {
        return None;
    }
    let base = polys.as_ptr() as *const u8;
    let ptrs: Vec<*const c_void> = (first..first + count).map(|i| unsafe { base.add(i * n * 32) } as *const c_void).collect();
    let mut out = vec![0u64; 12 * count];
    let rc = unsafe { sys::hm_msm_batch_bn256_g1_dev(handle, 0, ptrs.as_ptr(), n, count, ptr::null_mut(), out.as_mut_ptr()) };
    if rc != sys::HM_OK {
        return None;
    }
    Some(
        out.chunks_exact(12)
            .map(|w| {
                let mut xyz = [0u64; 12];
                xyz.copy_from_slice(w);
                g1_from_words(xyz)
            })
            .collect(),
    )
}

/// The same for ANY selection of the polynomials of a packed array (`indices[i]`: polynomial at [indices[i] n, (indices[i] + 1) n)):
/// every per-proof column of the table in one call, whatever lies between them.
pub fn commit_indexed_dev(handle: u64, polys: &DevicePoly, n: usize, indices: &[usize]) -> Option<Vec<G1>> {
    if indices.is_empty() {
        return Some(Vec::new());
    }
    if n == 0 || indices.iter().any(|&i| i.checked_add(1).map_or(true, |e| e.checked_mul(n).map_or(true, |e| e > polys.len()))) {
        return None;
    }
    let base = polys.as_ptr() as *const u8;
    let ptrs: Vec<*const c_void> = indices.iter().map(|&i| unsafe { base.add(i * n * 32) } as *const c_void).collect();
    let mut out = vec![0u64; 12 * indices.len()];
    let rc = unsafe { sys::hm_msm_batch_bn256_g1_dev(handle, 0, ptrs.as_ptr(), n, indices.len(), ptr::null_mut(), out.as_mut_ptr()) };
    if rc != sys::HM_OK {
        return None;
    }
    Some(
        out.chunks_exact(12)
            .map(|w| {
                let mut xyz = [0u64; 12];
                xyz.copy_from_slice(w);
                g1_from_words(xyz)
            })
            .collect(),
    )
}

/// halo2_proofs::arithmetic::eval_polynomial for `points.len()` polynomials of `n` coefficients lying back to back in `polys`
/// (polynomial q at point q): the Horner evaluations create_proof makes of every committed polynomial.
pub fn eval_polynomial_dev(polys: &DevicePoly, n: usize, points: &[Fr]) -> Option<Vec<Fr>> {
    if n == 0 || polys.len() < n * points.len() {
        return None;
    }
    let mut out: Vec<Fr> = Vec::with_capacity(points.len());
    let rc = unsafe {
        sys::hm_eval_polynomial_bn256_fr_dev(polys.as_ptr(), n, ptr::null(), points.as_ptr() as *const u64, points.len(), out.as_mut_ptr() as *mut u64, ptr::null_mut())
    };
    if rc != sys::HM_OK {
        return None;
    }
    unsafe { out.set_len(points.len()) };
    Some(out)
}

/// The UNDIVIDED numerator of h(X) -- custom gates, permutation and lookup terms combined by y -- as a straight-line program on
/// the device (hm_graph_create: five words per calculation, include/halo2_mi355x.h; halo2-experiments_amd/evaluation.py lowers
/// upstream's GraphEvaluator to it).  Built once per proving key.
#[derive(Debug)]
pub struct QuotientProgram {
    handle: u64,
    n_columns: usize,
    n_dynamic: usize,
}

impl QuotientProgram {
    pub fn new(calcs: &[[u32; 5]], constants: &[Fr], n_dynamic: usize, rotations: &[i32], n_columns: usize, n_intermediates: u32) -> Option<Self> {
        if !layout_ok() {
            return None;
        }
        let mut h = 0u64;
        let rc = unsafe {
            sys::hm_graph_create(calcs.as_ptr() as *const u32, calcs.len(), constants.as_ptr() as *const u64, constants.len(), n_dynamic,
                                 rotations.as_ptr(), rotations.len(), n_columns, n_intermediates, &mut h)
        };
        if rc != sys::HM_OK {
            return None;
        }
        Some(QuotientProgram { handle: h, n_columns, n_dynamic })
    }
    /// evaluate_h + divide_by_vanishing_poly + extended_to_coeff in ONE call: `columns[i]` = the n coefficients of entry i of the
    /// program's column table; `dynamic` = this proof's challenges, then beta, gamma, theta, y; `cosets` = indices of the cosets
    /// of the extended domain to evaluate on -- `domain.quotient_poly_degree` of them determine the quotient of a satisfied
    /// circuit (5 of 8 for the reference's circuits).  -> cosets.len() * n coefficients of h (piece t at [t n, (t + 1) n)).
    pub fn quotient_by_cosets(&self, domain: &DeviceDomain, columns: &[&DevicePoly], dynamic: &[Fr], cosets: &[usize]) -> Option<DevicePoly> {
        let n = domain.n();
        if columns.len() != self.n_columns || dynamic.len() != self.n_dynamic || cosets.is_empty() || columns.iter().any(|c| c.len() != n) {
            return None;
        }
        let ptrs: Vec<*const c_void> = columns.iter().map(|c| c.as_ptr()).collect();
        let mut shifts: Vec<u64> = Vec::with_capacity(4 * cosets.len());
        for &j in cosets {
            shifts.extend_from_slice(&words(&domain.coset_shift(j)));
        }
        let mut h = DevicePoly::new(cosets.len() * n)?;
        let w = words(&domain.omega);
        let rc = unsafe {
            sys::hm_quotient_by_cosets_bn256_fr_dev(self.handle, ptrs.as_ptr(), ptr::null(), ptrs.len(), dynamic.as_ptr() as *const u64, dynamic.len(), domain.k,
                                                    w.as_ptr(), shifts.as_ptr(), cosets.len(), cosets.len(), h.as_mut_ptr(), ptr::null_mut())
        };
        if rc == sys::HM_OK { Some(h) } else { None }
    }
    /// The same with the whole column table in ONE packed array (entry i at [i n, (i + 1) n)): what a prover that fills the table
    /// with `DevicePoly::upload_at` and transforms it with `lagrange_to_coeff_range` holds.
    pub fn quotient_by_cosets_packed(&self, domain: &DeviceDomain, table: &DevicePoly, dynamic: &[Fr], cosets: &[usize]) -> Option<DevicePoly> {
        let n = domain.n();
        if table.len() != self.n_columns * n || dynamic.len() != self.n_dynamic || cosets.is_empty() {
            return None;
        }
        let base = table.as_ptr() as *const u8;
        let ptrs: Vec<*const c_void> = (0..self.n_columns).map(|i| unsafe { base.add(i * n * 32) } as *const c_void).collect();
        let mut shifts: Vec<u64> = Vec::with_capacity(4 * cosets.len());
        for &j in cosets {
            shifts.extend_from_slice(&words(&domain.coset_shift(j)));
        }
        let mut h = DevicePoly::new(cosets.len() * n)?;
        let w = words(&domain.omega);
        let rc = unsafe {
            sys::hm_quotient_by_cosets_bn256_fr_dev(self.handle, ptrs.as_ptr(), ptr::null(), ptrs.len(), dynamic.as_ptr() as *const u64, dynamic.len(), domain.k,
                                                    w.as_ptr(), shifts.as_ptr(), cosets.len(), cosets.len(), h.as_mut_ptr(), ptr::null_mut())
        };
        if rc == sys::HM_OK { Some(h) } else { None }
    }
    /// Once per proving key: the values of the table entries `which` (the key's constant columns -- fixed, sigmas, l_0 / l_last /
    /// l_active, X -- whose coefficients lie in `table`) on `cosets`, in the form the program loads without a conversion product.
    /// -> which.len() x cosets.len() x n elements (entry w on coset c at [(w * cosets.len() + c) n, ...)), for
    /// `quotient_by_cosets_packed_kept`: those columns are then not transformed again in every proof (35 of 83 for MerkleSumTree).
    pub fn keep_on_cosets(&self, domain: &DeviceDomain, table: &DevicePoly, which: &[usize], cosets: &[usize]) -> Option<DevicePoly> {
        let n = domain.n();
        if table.len() != self.n_columns * n || cosets.is_empty() || cosets.len() > 16 || which.iter().any(|&i| i >= self.n_columns) {
            return None;
        }
        let mut shifts: Vec<u64> = Vec::with_capacity(4 * cosets.len());
        for &j in cosets {
            shifts.extend_from_slice(&words(&domain.coset_shift(j)));
        }
        let mut kept = DevicePoly::new(which.len() * cosets.len() * n)?;
        let w = words(&domain.omega);
        for (slot, &i) in which.iter().enumerate() {
            let src = unsafe { (table.as_ptr() as *const u8).add(i * n * 32) } as *const c_void;
            let dst = unsafe { (kept.as_mut_ptr() as *mut u8).add(slot * cosets.len() * n * 32) } as *mut c_void;
            if unsafe { sys::hm_coeff_to_cosets_bn256_fr_dev(src, dst, 1, w.as_ptr(), domain.k, shifts.as_ptr(), cosets.len(), 1, ptr::null_mut()) } != sys::HM_OK {
                return None;
            }
        }
        Some(kept)
    }
    /// `quotient_by_cosets_packed` with the columns `which` read from `kept` (what `keep_on_cosets` returned for the same `which` and
    /// `cosets`) instead of being transformed from their coefficients.
    pub fn quotient_by_cosets_packed_kept(&self, domain: &DeviceDomain, table: &DevicePoly, kept: &DevicePoly, which: &[usize], dynamic: &[Fr],
                                          cosets: &[usize]) -> Option<DevicePoly> {
        let n = domain.n();
        if table.len() != self.n_columns * n || dynamic.len() != self.n_dynamic || cosets.is_empty() || kept.len() != which.len() * cosets.len() * n
            || which.iter().any(|&i| i >= self.n_columns)
        {
            return None;
        }
        let base = table.as_ptr() as *const u8;
        let ptrs: Vec<*const c_void> = (0..self.n_columns).map(|i| unsafe { base.add(i * n * 32) } as *const c_void).collect();
        let mut pre: Vec<*const c_void> = vec![ptr::null(); self.n_columns];
        for (slot, &i) in which.iter().enumerate() {
            pre[i] = unsafe { (kept.as_ptr() as *const u8).add(slot * cosets.len() * n * 32) } as *const c_void;
        }
        let mut shifts: Vec<u64> = Vec::with_capacity(4 * cosets.len());
        for &j in cosets {
            shifts.extend_from_slice(&words(&domain.coset_shift(j)));
        }
        let mut h = DevicePoly::new(cosets.len() * n)?;
        let w = words(&domain.omega);
        let rc = unsafe {
            sys::hm_quotient_by_cosets_bn256_fr_dev(self.handle, ptrs.as_ptr(), pre.as_ptr(), ptrs.len(), dynamic.as_ptr() as *const u64, dynamic.len(), domain.k,
                                                    w.as_ptr(), shifts.as_ptr(), cosets.len(), cosets.len(), h.as_mut_ptr(), ptr::null_mut())
        };
        if rc == sys::HM_OK { Some(h) } else { None }
    }
}
impl Drop for QuotientProgram {
    fn drop(&mut self) {
        unsafe { sys::hm_graph_destroy(self.handle) };
    }
}
