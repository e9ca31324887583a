/*
 * halo2_mi355x.h -- C ABI of libhalo2_mi355x.so: the MI355X (gfx950) backend for the two
 * arithmetic kernels that dominate halo2_proofs::plonk::create_proof under KZG on BN256.
 *
 * What it replaces.  The reference (summa-dev/halo2-experiments) reaches this path only through
 * full_prover (/root/reference/src/circuits/utils.rs:22-70: ParamsKZG::setup :28, keygen_vk :31,
 * keygen_pk :35, create_proof :40-48), which runs the free functions of the halo2_proofs crate
 * pinned at /root/reference/Cargo.toml:10 (git tag v2023_02_02; source not vendored):
 *
 *     pub fn best_multiexp<C: CurveAffine>(coeffs: &[C::Scalar], bases: &[C]) -> C::Curve
 *     pub fn best_fft<G: Group>(a: &mut [G], omega: G::Scalar, log_n: u32)
 *
 * instantiated with C = bn256::G1Affine and G = bn256::Fr.  Those crates have no FFI; the
 * boundary below is what a `[patch]`-ed halo2_proofs::arithmetic would bind (INTEGRATION.md
 * shows the Rust side).  Each entry point names the upstream function it stands in for.
 *
 * Memory formats (halo2curves bn256) -- exactly the bytes Rust holds:
 *   Fr / Fq   4 x u64 little-endian limbs, Montgomery form (v * 2^256 mod m), fully reduced
 *   G1Affine  { x: Fq, y: Fq } = 8 x u64; the identity is (0, 0)
 *   G1        Jacobian { x, y, z: Fq } = 12 x u64; the identity has z = 0
 *
 * Conventions: every function returns HM_OK (0) or a negative HM_ERR_* code and never aborts or
 * throws across the boundary; hm_last_error() returns the message of the calling thread's last
 * failure.  Pointers are borrowed for the duration of the call only.  Calls are thread-safe (one
 * lock per device).  There is no CPU fallback inside this library: without a usable gfx950
 * device every compute entry point fails with HM_ERR_NO_DEVICE.
 */
#ifndef HALO2_MI355X_H
#define HALO2_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HM_OK 0
#define HM_ERR_BAD_ARG (-1)
#define HM_ERR_NO_DEVICE (-2)
#define HM_ERR_HIP (-3)
#define HM_ERR_NOT_FOUND (-4)
#define HM_ERR_INTERNAL (-5)
/* an in-place host-pointer call failed AFTER it began writing its result: the array is undefined (every other error
 * leaves the caller's arrays untouched, so a caller may fall back to its CPU body on them -- not after this one) */
#define HM_ERR_PARTIAL_OUTPUT (-6)
/* the input holds an invalid encoding or point (hm_g1_decompress_bn256*, hm_g1_check_bn256*): the smallest bad index is reported */
#define HM_ERR_INVALID_DATA (-7)

/* ---- lifecycle ---------------------------------------------------------------------------- */

/* Select the HIP device this thread's subsequent calls use (default: the current HIP device).
 * One process per GPU is the intended deployment; a single process may also drive several. */
int hm_set_device(int device);
/* Number of visible HIP devices (0 when there is none); never fails. */
int hm_device_count(void);
/* Free every device buffer, twiddle table and registered base set of the current device. */
int hm_shutdown(void);
/* Message of the last failure on the calling thread ("" if none). */
const char* hm_last_error(void);
/* Library version string. */
const char* hm_version(void);

/* ---- MSM: stands in for halo2_proofs::arithmetic::best_multiexp::<bn256::G1Affine> --------- */

/* sum_i scalars[i] * bases[i].  scalars: n x 4 u64 (Fr), bases: n x 8 u64 (G1Affine), both host
 * memory.  Result as an affine point (out_xy, Montgomery) plus an identity flag, which is the
 * canonical form of the G1 value best_multiexp returns; n == 0 yields the identity.
 * The scalars cross PCIe in every call.  The converted bases of the previous call are reused only when a
 * digest of the WHOLE base array (every word, 256 bits) and its length match -- never by pointer: a buffer
 * mutated at any index, or re-allocated at the same address with other contents, is uploaded again
 * (hm_set_host_base_cache(0) turns the reuse off altogether).  A caller that owns a long-lived base array --
 * ParamsKZG::g / g_lagrange -- still does best to register it once (below): that skips the digest too.
 * Largest call (every MSM form, per device): n * windows < 2^31 (point, window) item slots -- 2^27 points (12 windows
 * with the fixed-base table, 15 without); above that HM_ERR_BAD_ARG with a message, nothing computed.  A larger sum is
 * the hm_g1_sum of several calls over index ranges, or a split over devices (hm_set_msm_devices).  BASELINE's largest
 * configuration is 2^26. */
int hm_msm_bn256_g1(const uint64_t* scalars, const uint64_t* bases, size_t n, uint64_t out_xy[8], int* out_is_identity);

/* Same, Jacobian output (x, y, 1) / (0, 0, 0): the `C::Curve` value itself. */
int hm_msm_bn256_g1_jacobian(const uint64_t* scalars, const uint64_t* bases, size_t n, uint64_t out_xyz[12]);

/* Device-resident base sets (ParamsKZG::g / g_lagrange live for the whole proof):
 * upload + convert once, then run MSMs against bases[offset .. offset + n).
 * hm_release_bases never waits for the device: a set that an un-awaited hm_msm_submit_dev ticket still
 * reads is freed when that ticket is awaited, and the buffers of a released set are recycled by the next
 * registration of the same size. */
int hm_register_bases(const uint64_t* bases, size_t n, uint64_t* out_handle);
int hm_release_bases(uint64_t handle);
int hm_msm_bn256_g1_h(uint64_t handle, size_t offset, const uint64_t* scalars, size_t n, uint64_t out_xy[8],
                      int* out_is_identity);

/* Fixed-base variant for long-lived SRS sets (in halo2 the SRS is fixed for the life of the process:
 * /root/reference/src/circuits/utils.rs:28): additionally stores 2^(offset of window j) * P_i for every window j
 * (W x the memory: 12 GiB for 2^24 points -- sized for 288 GB of HBM; built once, ~0.22 s at 2^24), so that all
 * windows share ONE bucket set, the window grows from 17 to 22 bits and a fifth of the mixed additions disappears
 * (2^24 points: 19.5 ms against 21.5).  MSMs that cover the whole set (offset 0, n = set size) use the table; other
 * slices run the plain path on the same handle.  Results are identical either way. */
int hm_register_bases_precomp(const uint64_t* bases, size_t n, uint64_t* out_handle);
int hm_register_bases_precomp_dev(const void* d_bases, size_t n, void* stream, uint64_t* out_handle);
/* hm_register_bases / hm_register_bases_dev build that table BY THEMSELVES for sets of at least 2^log2_n points
 * (default 17: measured gains 4 % at 2^17, 13 % per dense commitment of a phase at 2^18, 3 % at 2^20 .. 2^22, 5 % at
 * 2^23, 9-15 % at 2^24, 15 % at 2^26; 0 = never, the plain layout only -- one copy of the points).  A phase of
 * commitments still sends its SPARSE columns (few surviving 256-row blocks) through the plain copy's five-launch plan.
 * Process-wide; read at registration time.  The environment variable HALO2_MI355X_FIXED_BASE_FROM_LOG sets the
 * initial value. */
int hm_set_fixed_base_threshold(uint32_t log2_n);
/* The PLAIN layout whatever the threshold says: one copy of the points, never a table.  For TRANSIENT sets -- a caller
 * that registers, runs one MSM and releases (the tensor form of the Python mirror's best_multiexp; a verifier's
 * commitments): building the table costs about ten MSMs of the same size (0.22 s and 12 GiB at 2^24 points). */
int hm_register_bases_plain(const uint64_t* bases, size_t n, uint64_t* out_handle);
int hm_register_bases_plain_dev(const void* d_bases, size_t n, void* stream, uint64_t* out_handle);

/* What a registration ended up with.  hm_register_bases / _dev fall back to the plain layout when the W copies of the
 * table cannot be allocated (after giving the parked buffers of released sets back to the allocator and trying once
 * more): the call still succeeds, table_windows == 0 tells, and default_tables_dropped counts such registrations of
 * the process.  A multi-device handle (hm_set_msm_devices) reports sums over its parts. */
typedef struct hm_bases_info {
  uint64_t n;                      /* points of the set */
  uint64_t device_bytes;           /* HBM the set holds (all devices) */
  uint64_t parked_bytes;           /* buffers of RELEASED sets kept for reuse on the set's device(s) (at most 2 GiB each) */
  uint64_t default_tables_dropped; /* process-wide: default registrations that fell back to the plain layout */
  uint32_t table_windows;          /* 0: plain layout; else the W of the fixed-base table */
  uint32_t table_window_bits;      /* the table's widest window */
  uint32_t devices;                /* 1, or the parts of a multi-device handle */
  uint32_t sliced;                 /* multi-device: 1 = index-range slices, 0 = replicas */
} hm_bases_info;
int hm_get_bases_info(uint64_t handle, hm_bases_info* out);

/* Device-pointer forms (inputs already in HBM; `stream` is a hipStream_t or NULL).  The result is
 * written to host memory, so the call synchronises `stream` before returning. */
int hm_register_bases_dev(const void* d_bases, size_t n, void* stream, uint64_t* out_handle);
int hm_msm_bn256_g1_dev(uint64_t handle, size_t offset, const void* d_scalars, size_t n, void* stream,
                        uint64_t out_xyz[12]);

/* Asynchronous form: enqueue the whole MSM on `stream` and return a ticket at once (up to 8 MSMs in
 * flight per device, each with its own workspace); hm_msm_wait blocks on that MSM only, folds and
 * returns its result.  Independent commitments issued on different streams overlap: one MSM's
 * latency-bound phases (sort, bucket reduction, host fold) hide behind another's accumulation. */
int hm_msm_submit_dev(uint64_t handle, size_t offset, const void* d_scalars, size_t n, void* stream, uint64_t* out_ticket);
int hm_msm_wait(uint64_t ticket, uint64_t out_xyz[12]);
/* The commitments of one prover phase in one call (create_proof commits its advice / lookup / permutation columns in
 * loops of independent commit_lagrange calls): `count` scalar arrays of n elements each (d_scalars: host array of device
 * pointers, produced on `stream`) against bases[offset .. offset + n); out_xyz: count x 12 u64, in call order.  The library
 * keeps eight MSMs in flight on streams of its own; the call returns when all results are on the host. */
int hm_msm_batch_bn256_g1_dev(uint64_t handle, size_t offset, const void* const* d_scalars, size_t n, size_t count, void* stream,
                              uint64_t* out_xyz);
/* The same with the scalar arrays in HOST memory (scalars: host array of `count` host pointers, n x 4 u64 each) -- what a
 * prover that still keeps its polynomials in host vectors calls per phase: every chain's upload runs on its own stream,
 * so the PCIe time of one commitment hides behind the kernels of the others. */
int hm_msm_batch_bn256_g1_h(uint64_t handle, size_t offset, const uint64_t* const* scalars, size_t n, size_t count, uint64_t* out_xyz);

/* Single-process multi-GPU best_multiexp (the form a Rust prover, one process for the whole node,
 * binds): after hm_set_msm_devices(devices, count >= 2) every hm_msm_bn256_g1 /
 * hm_msm_bn256_g1_jacobian call splits [0, n) into `count` contiguous index ranges, runs one range per
 * listed device from its own host thread (each device caches its slice of the SRS exactly as the
 * one-device path does) and folds the 96-byte partial results on the host -- the data path has no
 * inter-GPU exchange.  Inputs below 2^14 points per device go whole to devices[0].  count == 0
 * restores the default (the calling thread's current device).  Replaces the same call sites as
 * hm_msm_bn256_g1 (halo2_proofs::arithmetic::best_multiexp). */
int hm_set_msm_devices(const int* devices, int count);

/* Sum of `count` G1 values (12 x u64 each, z = 0 for the identity), normalised to (x, y, 1): the
 * fold of per-GPU partial results of a sharded best_multiexp after the RCCL all-gather.  Pure host
 * arithmetic on a handful of points (the exchange is ~96 B per rank); needs no device. */
int hm_g1_sum(const uint64_t* points_xyz, size_t count, uint64_t out_xyz[12]);

/* enable != 0 (default): hm_msm_bn256_g1* may reuse the previous call's converted bases when the full-content digest
 * matches; 0: always upload and convert. */
int hm_set_host_base_cache(int enable);

/* ---- device memory for callers without a HIP binding of their own -------------------------------------------------
 * Everything a Rust (or C) prover needs to keep its polynomials in HBM between the steps of create_proof and use the *_dev
 * entry points with nothing but this library (rust/halo2_proofs-patch/src/mi355x_dev.rs: DevicePoly).  All on the calling
 * thread's current device (hm_set_device).
 *   hm_device_malloc / hm_device_free: hipMalloc / hipFree (free waits for the device: keep buffers for the life of a proof);
 *   hm_copy_to_device / hm_copy_to_host: synchronous, through the same copy policy as the host-pointer forms (hm_set_host_copies).
 *     Ordered behind everything queued on the device's default stream and on blocking streams (the call waits for them, whichever
 *     way the bytes travel); work on NON-blocking streams of the caller's own needs the caller's synchronisation first
 *     (hm_device_synchronize() waits for all streams).  stream == NULL in the *_dev entry points is the device's default stream. */
int hm_device_malloc(size_t bytes, void** d_out);
int hm_device_free(void* d_ptr);
int hm_copy_to_device(void* d_dst, const void* src, size_t bytes);
int hm_copy_to_host(void* dst, const void* d_src, size_t bytes);
/* `count` arrays in ONE call: srcs[i] -> d_dsts[i] (resp. d_srcs[i] -> dsts[i]), bytes[i] each.  The copy lanes treat them as one
 * transfer -- the columns of a proof (48 x 8 MiB at k = 18) move at the rate of one 384 MiB array instead of 48 small ones, each with
 * its own helper threads, pipeline fill and drain.  Same ordering and error convention as the single forms; a failure of the
 * _to_host form may leave any of the destinations partly written (HM_ERR_PARTIAL_OUTPUT). */
int hm_copy_many_to_device(void* const* d_dsts, const void* const* srcs, const size_t* bytes, size_t count);
int hm_copy_many_to_host(void* const* dsts, const void* const* d_srcs, const size_t* bytes, size_t count);
int hm_device_synchronize(void);

/* How the host-pointer forms move their arrays (csrc/xfer.hip) -- a rule on the host RANGE, never on a timing.
 * 0 = auto (the default; HALO2_MI355X_HOST_COPIES sets the start value): a range the caller has declared long-lived with
 *     hm_host_register goes straight to hipMemcpy (a DMA from registered memory); every other range of 256 KiB or more goes through the
 *     library's own pinned staging lanes -- nothing of the caller's memory is handed to the driver, so the cost does not depend on what
 *     pinning a page costs on the box (0.1 us or 9 us: both exist in one pool) nor on what the caller maps and unmaps around the calls;
 * 1 = lanes always (registered ranges too); 2 = direct always (hipMemcpy pins the caller's pages on the fly: 0.2 ms per 64 MiB
 *     faster where pinning is cheap, 2.3 ms per MiB slower where it is not -- for boxes known to pin fast).  Process-wide. */
int hm_set_host_copies(int mode);
/* Declare [p, p + bytes) long-lived host memory (an SRS kept in memory, a staging buffer reused for every proof): pinned ONCE here
 * (hipHostRegister, portable across devices), after which the host-pointer forms and hm_copy_to_* DMA from / into it directly.  The
 * range must stay mapped until hm_host_unregister(p) (p = the start of a registered range); ranges must not overlap.  Needs a
 * device (the registration is the runtime's).  Not for arrays that live for one call: registering costs what the lanes avoid. */
int hm_host_register(const void* p, size_t bytes);
int hm_host_unregister(const void* p);

/* Window-size override for experiments (0 = automatic). */
int hm_msm_set_window(int c);
/* Per-phase timing of an MSM (digits / sort / accumulate / reduce and the accumulate kernel alone, reported by
 * hm_get_msm_stats) costs seven event records per call.  mode -1 (default): the general pipeline (n >= 2^19 and
 * precomputed sets) records them, the five-launch plan of prover sizes records only the total; 0: never; 1: always. */
int hm_msm_set_phase_timing(int mode);

/* ---- NTT: stands in for halo2_proofs::arithmetic::best_fft::<bn256::Fr> --------------------- */

/* In place on host memory: a[j] <- sum_i a[i] * omega^(i*j), natural order in and out, unscaled.
 * a: 2^log_n x 4 u64 (Fr); omega: 4 u64 (Fr), a 2^log_n-th root of unity; log_n <= 28.
 * `a` is written only by the final copy from the device: every error code but HM_ERR_PARTIAL_OUTPUT (that copy itself
 * failed) leaves it exactly as it was. */
int hm_ntt_bn256_fr(uint64_t* a, const uint64_t omega[4], uint32_t log_n);

/* Device-pointer form, in place, asynchronous on `stream`.  Every *_dev NTT entry point may be called
 * concurrently on different streams (and from different threads): the ping-pong buffer of a multi-pass
 * transform belongs to the stream in use (a small pool, handed over behind an event), fused constants
 * travel to the kernels by value, and twiddle tables built on one stream are published to the others
 * behind an event.
 * Every *_dev NTT entry point below (hm_ntt*, hm_ifft, hm_coset_ntt, hm_coeff_to_extended, hm_extended_to_coeff, hm_coeff_to_coset(s),
 * hm_coset(s)_to_coeff) refuses with HM_ERR_BAD_ARG, before anything is launched and without needing a device: a null argument,
 * log_n (log_ext) > 28, log_n > log_ext, more than 16 cosets, batch or batch * cosets > 65535, an output overlapping its input where
 * the form is out of place, and a DATA POINTER THAT IS NOT 16-BYTE ALIGNED (the passes move an element as two 16-byte halves). */
int hm_ntt_bn256_fr_dev(void* d_a, const uint64_t omega[4], uint32_t log_n, void* stream);

/* `batch` back-to-back arrays of 2^log_n elements transformed by ONE set of launches (the ~48
 * same-size transforms of a proof).  scale (4 words) and coset (12 words) are
 * optional (NULL): the fused EvaluationDomain::ifft divisor and the coeff_to_extended coset shift. */
int hm_ntt_batch_bn256_fr_dev(void* d_a, size_t batch, const uint64_t omega[4], uint32_t log_n, const uint64_t* scale,
                              const uint64_t* coset, void* stream);

/* ---- next rows: the EvaluationDomain steps either side of best_fft ----------- */

/* EvaluationDomain::ifft: best_fft(a, omega_inv, log_n) then a[i] *= divisor, with the scaling
 * fused into the last NTT pass.  Device pointers, in place. */
int hm_ifft_bn256_fr_dev(void* d_a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4], void* stream);
/* EvaluationDomain::coeff_to_extended's arithmetic: a[i] *= coset[i % 3] (distribute_powers_zeta
 * with coset = {1, g, g^2}) fused into the first pass of best_fft(a, omega_ext, log_n).
 * The caller has already zero-padded a to 2^log_n. */
int hm_coset_ntt_bn256_fr_dev(void* d_a, const uint64_t omega[4], uint32_t log_n, const uint64_t coset[12], void* stream);
/* EvaluationDomain::coeff_to_extended in one call (halo2_proofs poly/domain.rs: resize to the extended
 * domain with zeros, distribute_powers_zeta, best_fft with extended_omega): `batch` compact coefficient
 * arrays of 2^log_n x 32 B at d_coeffs -> `batch` arrays of 2^log_ext evaluations at d_ext (out of
 * place, d_ext need not be initialised).  coset = {1, zeta, zeta^2} as for hm_coset_ntt_bn256_fr_dev,
 * or NULL.  The zero-padded part is never materialised: the first pass reads only the coefficients, and
 * the log_ext - log_n butterfly stages that would pair them with zeros cost nothing. */
int hm_coeff_to_extended_bn256_fr_dev(const void* d_coeffs, void* d_ext, size_t batch, const uint64_t extended_omega[4],
                                      uint32_t log_n, uint32_t log_ext, const uint64_t* coset, void* stream);
/* The extended domain one coset of the n-th roots of unity at a time.  The 2^log_ext points zeta * extended_omega^m that
 * coeff_to_extended evaluates on fall into E = 2^(log_ext - log_n) cosets shift_j * <omega>, shift_j = zeta *
 * extended_omega^j, omega = extended_omega^E: row m = E t + j of the extended array is point t of coset j.  A rotation of
 * the circuit (X -> omega^rot X) stays inside a coset, and 1 / (X^n - 1) is ONE constant on it, so evaluate_h runs on each
 * coset by itself (hm_graph_evaluate_dev over 2^log_n rows, rotations unscaled) -- E independent n-point problems that can
 * go to E different GPUs, each needing only the coefficient arrays (later versions of halo2_proofs take the same route
 * for memory: coeff_to_extended_part).
 *   hm_coeff_to_coset:  d_out_b[t] = sum_i d_coeffs_b[i] (shift omega^t)^i for `batch` back-to-back arrays of 2^log_n Fr
 *     (= row E t + j of hm_coeff_to_extended's output, bit for bit); d_out may be d_coeffs itself.  columns_internal != 0:
 *     outputs multiplied by 32, the form HM_GRAPH_COLUMNS_INTERNAL loads.  The powers of `shift` are kept on the device
 *     per (shift, log_n).
 *   hm_coset_to_coeff:  in place, a_b <- divisor * (inverse transform with omega_inv) of a_b, then a_b[i] *= shift_inv^i:
 *     with divisor = 1/n this is d_j[i] = sum_q h[i + q n] zeta^(n q) w^(j q) (w = extended_omega^n, a primitive E-th
 *     root of unity) for the coefficients h of the polynomial whose values on coset j went in; the E of them recombine as
 *     h[i + q n] = zeta^(-n q) / E * sum_j w^(-j q) d_j[i] (hm_fr_linear_combination_dev, E terms per q).
 * Asynchronous on `stream`. */
int hm_coeff_to_coset_bn256_fr_dev(const void* d_coeffs, void* d_out, size_t batch, const uint64_t omega[4], uint32_t log_n,
                                   const uint64_t shift[4], int columns_internal, void* stream);
int hm_coset_to_coeff_bn256_fr_dev(void* d_a, size_t batch, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4],
                                   const uint64_t shift_inv[4], void* stream);
/* Several cosets in one launch chain (at most 16 per call).
 *   hm_coeff_to_cosets: d_out holds batch * count arrays of 2^log_n Fr; array b * count + c = coefficient array b evaluated
 *     on the coset shifts[c] * <omega> -- per input the `count` cosets lie one after the other, which is the column layout
 *     hm_graph_evaluate_segments_dev reads (segment c = coset c).  shifts: host, count x 4 u64.  d_out must not overlap d_coeffs.
 *   hm_cosets_to_coeff: in place on `count` back-to-back arrays (the values of ONE polynomial on `count` cosets): array c
 *     <- divisor * inverse transform, then element i *= shift_invs[c]^i.
 * Only j - 1 of the E cosets are needed for the quotient of a satisfied circuit (it has fewer than n (j - 1) coefficients):
 * partial_c[i] = sum_t h[i + t n] u_c^t with u_c = shifts[c]^n is a (j - 1) x (j - 1) Vandermonde system per i, whose
 * inverse matrix -- times 1 / (u_c - 1), the vanishing polynomial's inverse on coset c, if the numerator was evaluated
 * undivided -- gives every piece of h as ONE hm_fr_linear_combination_dev of the partials. */
int hm_coeff_to_cosets_bn256_fr_dev(const void* d_coeffs, void* d_out, size_t batch, const uint64_t omega[4], uint32_t log_n,
                                    const uint64_t* shifts, size_t count, int columns_internal, void* stream);
int hm_cosets_to_coeff_bn256_fr_dev(void* d_a, size_t count, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4],
                                    const uint64_t* shift_invs, void* stream);

/* EvaluationDomain::extended_to_coeff's arithmetic in one call (halo2_proofs poly/domain.rs: ifft over the
 * extended domain, then distribute_powers_zeta with the INVERSE coset powers): `batch` arrays of 2^log_ext
 * evaluations, in place; best_fft(a, extended_omega_inv, log_ext), then a[i] *= divisor * coset_inv[i % 3]
 * with coset_inv = {1, zeta^-1, zeta^-2} -- divisor and pattern are folded into three constants that the
 * LAST NTT pass multiplies in, so no separate sweep over the 2^log_ext elements remains.  The caller
 * truncates to n * (j - 1) coefficients. */
int hm_extended_to_coeff_bn256_fr_dev(void* d_a, size_t batch, const uint64_t extended_omega_inv[4], uint32_t log_ext,
                                      const uint64_t divisor[4], const uint64_t coset_inv[12], void* stream);

/* Host-pointer forms of the two steps above, for a prover whose polynomials stay in host memory (the drop-in patch of
 * rust/halo2_proofs-patch: EvaluationDomain::coeff_to_extended / extended_to_coeff, halo2_proofs poly/domain.rs).  Only what
 * upstream's arrays really hold crosses PCIe:
 *   hm_coeff_to_extended_bn256_fr: coeffs = 2^log_n x 4 u64 in (the zero padding upstream's `resize` appends is never uploaded),
 *     ext = 2^log_ext x 4 u64 out; coset = {1, zeta, zeta^2} (12 words) or NULL.  `ext` is written by the final copy alone and
 *     may be the allocation `coeffs` lives in (upstream resizes its Vec in place): every error code but HM_ERR_PARTIAL_OUTPUT
 *     leaves both arrays as they were.
 *   hm_extended_to_coeff_bn256_fr: a = 2^log_ext x 4 u64 evaluations in; the first `keep` coefficients (keep <= 2^log_ext:
 *     upstream truncates to n * (j - 1)) come back into a[0 .. keep), the rest of `a` keeps its old contents -- the caller
 *     truncates.  Same error contract.
 * Synchronous; run on the calling thread's current device (the library's own stream). */
int hm_coeff_to_extended_bn256_fr(const uint64_t* coeffs, uint64_t* ext, const uint64_t extended_omega[4], uint32_t log_n,
                                  uint32_t log_ext, const uint64_t* coset);
int hm_extended_to_coeff_bn256_fr(uint64_t* a, size_t keep, const uint64_t extended_omega_inv[4], uint32_t log_ext,
                                  const uint64_t divisor[4], const uint64_t coset_inv[12]);

/* halo2_proofs::arithmetic::eval_polynomial (the Horner evaluations create_proof makes of every committed
 * polynomial at x * omega^rot): out[q] = sum_i poly_q[i] * points[q]^i for q < count, where poly_q is the
 * coefficient array number poly_index[q] (or q when poly_index is NULL) of the back-to-back arrays of n Fr at
 * d_polys.  points and out are host memory (count x 4 u64); the call synchronises `stream`. */
int hm_eval_polynomial_bn256_fr_dev(const void* d_polys, size_t n, const uint32_t* poly_index, const uint64_t* points, size_t count,
                                    uint64_t* out, void* stream);

/* halo2_proofs::arithmetic::kate_division(a, z): the quotient of a(X) - a(z) by X - z, which multiopen builds for
 * every opening (upstream poly/kzg/multiopen; reached from /root/reference/src/circuits/utils.rs:40-48).  d_poly: n
 * coefficients, d_quotient: n - 1 coefficients (q[i] = a[i+1] + z q[i+1]); the two must not overlap.  n < 2 writes
 * nothing.  Asynchronous on `stream`. */
int hm_kate_division_bn256_fr_dev(const void* d_poly, size_t n, const uint64_t z[4], void* d_quotient, void* stream);

/* `count` such divisions in one launch chain (the quotients one multiopen round builds are independent of each other):
 * d_polys / d_quotients: host arrays of `count` device pointers (n resp. n - 1 coefficients each), z: host, count x 4
 * u64, one point per polynomial.  No quotient may overlap any polynomial of the call.  Same results as `count` calls of
 * the form above.  Asynchronous on `stream`. */
int hm_kate_division_batch_bn256_fr_dev(const void* const* d_polys, size_t n, const uint64_t* z, void* const* d_quotients, size_t count,
                                        void* stream);

/* The running products of the permutation and lookup arguments (upstream plonk/permutation/prover.rs and
 * plonk/lookup/prover.rs: z[0] = start, z[row] = z[row - 1] * factors[row - 1]): d_out[i] = start * prod_{j < i}
 * d_factors[j] for i < n.  d_out may be d_factors itself.  Asynchronous on `stream`. */
int hm_fr_grand_product_dev(const void* d_factors, size_t n, const uint64_t start[4], void* d_out, void* stream);

/* The z columns of one argument in one launch chain.  d_factors / d_out: host arrays of `count` device pointers (n
 * elements each; d_out[j] may be d_factors[j] itself, and must not overlap any other column of the call).
 *   chain_row >= n (HM_NO_CHAIN): every column starts from `start` -- the lookup arguments' products (upstream
 *     plonk/lookup/prover.rs, one z per lookup, each from 1);
 *   chain_row <  n: column 0 starts from `start` and column j + 1 from d_out[j][chain_row] -- upstream's `last_z`
 *     (plonk/permutation/prover.rs: the z of a column set starts where the set before stood at the last usable row,
 *     chain_row = n - (blinding_factors + 1)); nothing is read back between the columns.
 * Same results as `count` calls of the form above made in order.  Asynchronous on `stream`. */
#define HM_NO_CHAIN ((size_t)-1)
int hm_fr_grand_product_batch_dev(const void* const* d_factors, size_t n, const uint64_t start[4], size_t chain_row, void* const* d_out,
                                  size_t count, void* stream);

/* ff::BatchInvert::batch_invert on n device-resident elements, in place: every non-zero element is replaced by its
 * inverse, zero stays zero (the denominators of the grand products above).  Asynchronous on `stream`. */
int hm_fr_batch_invert_dev(void* d_values, size_t n, void* stream);

/* d_out[i] = sum_{j < count} coeffs[j] * d_polys[j][i] for i < n: `Polynomial * scalar` and `+` of upstream
 * poly.rs in one pass (the random linear combinations of multiopen, the pieces of h(X)).  d_polys: host array of
 * `count` device pointers (n x 4 u64 each); coeffs: host, count x 4 u64.  d_out may be one of the inputs (the same
 * pointer, not a shifted view).  count = 0 zeroes d_out.  Asynchronous on `stream`. */
int hm_fr_linear_combination_dev(const void* const* d_polys, const uint64_t* coeffs, size_t count, size_t n, void* d_out,
                                 void* stream);

/* The set quotient of the SHPLONK multiopen (upstream poly/kzg/multiopen/shplonk/prover.rs): for one rotation set with the
 * t distinct points `points` and N(X) = sum_{j < m} weights[j] * d_polys[j](X),
 *     d_out[i] (+)= scale * ((N - R) / prod_l (X - points[l]))[i]   for i < n - t,     deg R < t, R(points[l]) = N(points[l]),
 * the same words upstream's interpolate / subtract / divide chain gives.  It is computed as sum_l c_l * kate_division(N,
 * points[l]) with c_l = 1 / prod_{l' != l} (points[l] - points[l']): t scans over one read of N, no R, no evaluation.  t = 1 is
 * scale * kate_division(N, points[0]), the multiopen's final quotient.
 *   d_polys: host array of m device pointers (n x 4 u64 each, 16-byte aligned, canonical); weights: host, m x 4 u64; points:
 *   host, t x 4 u64; scale: host, 4 u64 (all canonical Montgomery words); d_out: n x 4 u64 on the device.
 *   accumulate = 0: rows [0, n - t) are written and rows [n - t, n) are written as zero;  != 0: the quotient is added to rows
 *   [0, n - t) and the rows above (to which it adds zero) are left alone.  d_out may be one of d_polys.
 * HM_ERR_BAD_ARG, with d_out untouched: a null or misaligned pointer, m = 0, t = 0, t > HM_SHPLONK_MAX_POINTS, n < t + 1, two
 * equal points, a point or the scale not below r.  Scratch (N and the scans' carries) is allocated and freed in stream order;
 * nothing is read back.  Asynchronous on `stream`. */
#define HM_SHPLONK_MAX_POINTS 4
int hm_shplonk_set_quotient_bn256_fr_dev(const void* const* d_polys, const uint64_t* weights, size_t m, size_t n, const uint64_t* points,
                                         size_t t, const uint64_t scale[4], void* d_out, int accumulate, void* stream);

/* The two entries above for a batch of `proofs` INDEPENDENT proofs of one structure (count / m, t and n the same for all, the values
 * each proof's own), word for word the loop of the single entry over b, as ONE launch chain whose grid has a proof dimension:
 *   d_polys: host array of proofs x count (proofs x m) device pointers, proof b's at [b * count, (b + 1) * count); the same pointer may
 *   occur in several proofs (the fixed and permutation polynomials of a proving key do);  coeffs / weights: host, proofs x count x 4 u64;
 *   points: host, proofs x t x 4 u64;  scales: host, proofs x 4 u64;  d_outs: host array of `proofs` device pointers.
 * The per-proof coefficients, points and partial fractions travel in a device table uploaded with the call, and all proofs share one
 * stream-ordered workspace allocation.  d_outs[b] may be one of proof b's own inputs.  HM_ERR_BAD_ARG with nothing launched and every
 * output untouched: what the single entry refuses, in any proof; d_outs[b] equal to another proof's input or output; proofs = 0
 * (set quotient) or proofs > 65535.  Asynchronous on `stream`. */
int hm_fr_linear_combination_batch_dev(const void* const* d_polys, const uint64_t* coeffs, size_t count, size_t n, void* const* d_outs,
                                       size_t proofs, void* stream);
int hm_shplonk_set_quotient_batch_bn256_fr_dev(const void* const* d_polys, const uint64_t* weights, size_t m, size_t n, const uint64_t* points,
                                               size_t t, const uint64_t* scales, void* const* d_outs, int accumulate, size_t proofs,
                                               void* stream);

/* The permuted columns of one lookup argument (upstream plonk/lookup/prover.rs: permute_expression_pair): from the first
 * `rows` (= usable rows) entries of the compressed input and table columns, d_permuted_input[0 .. rows) = the input values
 * sorted by their canonical integers, d_permuted_table[0 .. rows) = the table values arranged so that every row where the
 * sorted input changes holds that input value and the leftover table values fill the repeated rows (ascending values from
 * the last such row backwards, exactly as upstream walks them).  The blinding rows beyond `rows` are the caller's.  The
 * outputs must not overlap the inputs.  Returns HM_ERR_NOT_FOUND when an input value does not occur in the table
 * (upstream: Error::ConstraintSystemFailure).  Synchronises `stream`. */
int hm_lookup_permute_bn256_fr_dev(const void* d_input, const void* d_table, size_t rows, void* d_permuted_input,
                                   void* d_permuted_table, void* stream);
/* The same for the `count` lookup arguments of a circuit at once (create_proof maps commit_permuted over them): one launch
 * chain carries up to eight lookups, so their 256-bit sorts run side by side.  Host arrays of `count` device pointers;
 * missing (optional, count ints) is set to 1 for every lookup whose input holds a value its table lacks. */
int hm_lookup_permute_batch_bn256_fr_dev(const void* const* d_inputs, const void* const* d_tables, size_t count, size_t rows,
                                         void* const* d_permuted_inputs, void* const* d_permuted_tables, int* missing, void* stream);

/* The multiplicity columns of `count` logUp lookup arguments (the logarithmic-derivative lookup; this project's own proof format,
 * DESIGN.md section 33) in one call.  Argument a has the table column d_tables[a] and input_counts[a] >= 1 input columns, its
 * entries of d_inputs (a flat host array of sum(input_counts) device pointers, argument a's behind those of the arguments before
 * it); of every column the first `rows` (= usable rows) entries are read, canonical Montgomery words, 16-byte aligned.
 *     d_m[a][i] = the number of (input column, row) pairs of argument a whose value is d_tables[a][i], when i is the first row of
 *                 the table holding that value, and 0 on the later rows that repeat it            for i < rows, Montgomery words.
 * Nothing is sorted when every table value of the call is an integer below 2^20 (value bins); otherwise each table goes through
 * the record sort of hm_fr_argsort_bn256_dev (then rows <= 2^26) and the inputs are searched in it.  The blinding rows beyond
 * `rows` are the caller's.  missing (optional, count ints) is set to 1 for every argument one of whose inputs holds a value its
 * table lacks, and the call then returns HM_ERR_NOT_FOUND (upstream: Error::ConstraintSystemFailure); the d_m of the other
 * arguments are complete.  HM_ERR_BAD_ARG with nothing launched: a null or misaligned pointer, rows = 0 or >= 2^31, an
 * input_counts[a] of 0 or with input_counts[a] * rows >= 2^32 (the counters are 32-bit), a d_m that overlaps any other column
 * of the call.  Synchronises `stream`. */
int hm_logup_multiplicities_bn256_fr_dev(const void* const* d_tables, const void* const* d_inputs, const uint32_t* input_counts, size_t count,
                                         size_t rows, void* const* d_m, int* missing, void* stream);

/* The running sums of the logUp arguments: d_out[c][i] = sum_{j < i} d_terms[c][j] mod r for i < n (exclusive: d_out[c][0] = 0),
 * for `count` columns of n canonical Montgomery elements in one launch chain of three launches.  d_terms / d_out: host arrays of
 * `count` device pointers, 16-byte aligned; d_out[c] may be d_terms[c] itself and must not overlap any other column of the call.
 * HM_ERR_BAD_ARG with nothing launched: a null or misaligned pointer, n = 0 or >= 2^32, count > 65535, an overlap.  Scratch (the
 * block totals) is allocated and freed in stream order.  Asynchronous on `stream`. */
int hm_fr_grand_sum_batch_dev(const void* const* d_terms, size_t n, void* const* d_out, size_t count, void* stream);

/* d_a[i] *= pattern[i mod period] for i < n, in place: EvaluationDomain::divide_by_vanishing_poly (upstream poly/domain.rs:
 * on the extended coset 1 / (X^n - 1) takes only 2^(extended_k - k) values, t_evaluations).  pattern: host, period x 4 u64;
 * period a power of two <= 64.  Asynchronous on `stream`. */
int hm_fr_mul_periodic_dev(void* d_a, size_t n, const uint64_t* pattern, uint32_t period, void* stream);

/* out[i] = x^i for i < n (device pointer, n x 4 u64): the ladder 1, s, s^2, ... of ParamsKZG::setup, whose
 * fixed-base multiples are g, and whose scaled inverse NTT gives the Lagrange-basis scalars of g_lagrange. */
int hm_fr_powers_dev(void* d_out, size_t n, const uint64_t x[4], void* stream);

/* evaluate_h's gate arithmetic (halo2_proofs::plonk::evaluation::GraphEvaluator): a circuit's gate / lookup
 * expressions, flattened into a straight-line program, run once per row of the extended domain with every column
 * resident in HBM.  A calculation is five words { op, a, b, c, target }:
 *   op      0 Add  1 Sub  2 Mul  3 Square  4 Double  5 Negate  6 Store  7 MulAdd (a * b + c: one Horner step)
 *   a b c   value sources: kind << 30 | rotation_index << 20 | index, with kind 0 Constant(index), 1 Intermediate(index),
 *           2 Column(index & 0x3fff) at row (idx + rotations[rotation_index]) mod 2^log_size, 3 PreviousValue (d_values[idx] on entry)
 *   target  the intermediate this calculation defines (each is written exactly once, as upstream's are)
 * Upstream's Fixed / Advice / Instance queries are entries of one column table.  Constants [0, n_const) belong to the
 * program (the circuit's); constants [n_const, n_const + n_dynamic) are given with every call -- upstream's Challenge /
 * Beta / Gamma / Theta / Y sources, which change with every proof (n_dynamic <= 16).  Horner(start, parts, factor) is a
 * chain of MulAdd.  rotations are in ROWS (upstream's rot * 2^(extended_k - k)).  The value of the program is its last
 * calculation's (upstream GraphEvaluator::evaluate); it is written to d_values[idx] (2^log_size x 4 u64, external words).
 * A Column source may name a column SHORTER than the domain: index = column | log2(rows) << 14 reads it at the row index
 * modulo its 2^log2(rows) rows (log2(rows) = 0: a full-size column; the table holds at most 256 columns) -- the inverse
 * vanishing-polynomial pattern of divide_by_vanishing_poly (period 2^(extended_k - k)) is such a column, so the division is
 * the program's last multiplication.
 * hm_graph_create validates the program, assigns intermediates to a minimal number of slots by liveness and uploads it;
 * evaluation is asynchronous on `stream` and may run concurrently on different streams.  d_values and every column pointer
 * must be 16-byte aligned (a cell is moved as two 16-byte halves): one that is not is refused with HM_ERR_BAD_ARG, by
 * hm_graph_evaluate_dev, hm_graph_evaluate_flags_dev and hm_graph_evaluate_segments_dev alike. */
int hm_graph_create(const uint32_t* calcs, size_t n_calc, const uint64_t* constants, size_t n_const, size_t n_dynamic,
                    const int32_t* rotations, size_t n_rot, size_t n_columns, uint32_t n_intermediates, uint64_t* out_handle);
int hm_graph_evaluate_dev(uint64_t handle, const void* const* d_columns, size_t n_columns, const uint64_t* dynamic_constants,
                          size_t n_dynamic, uint32_t log_size, void* d_values, void* stream);
/* The quotient h(X) of a proof in ONE call, from COEFFICIENT arrays -- what upstream's evaluate_h, divide_by_vanishing_poly and
 * extended_to_coeff make of the extended arrays (halo2_proofs plonk/evaluation.rs, poly/domain.rs; reached from
 * /root/reference/src/circuits/utils.rs:40-48).
 *   program: an hm_graph_create handle of the UNDIVIDED numerator (custom gates, permutation and lookup terms combined by y)
 *     with rotations as on the n-row domain (unscaled) and every entry of its column table a polynomial of n coefficients;
 *   d_coeff_columns: n_columns device pointers, 2^log_n coefficients each (fixed, then advice, then instance -- the
 *     identity polynomial X where the program reads the point itself);
 *   d_on_cosets: NULL, or n_columns entries of which the non-NULL ones name columns whose values on the `count` cosets exist
 *     already -- count x 2^log_n words as hm_coeff_to_cosets_bn256_fr_dev(..., columns_internal = 1) wrote them for the same
 *     shifts (the fixed columns, permutation polynomials and l_0 / l_last / l_active of a proving key: transformed once, not
 *     once per proof); d_coeff_columns[i] is then not read;
 *   shifts: host, count x 4 u64 -- the cosets shift_c * <omega> to evaluate on, shift_c = zeta * extended_omega^(j_c), distinct
 *     and outside the n-th roots; `count` >= `pieces`, and pieces = (max degree - 1) cosets determine the quotient of a satisfied
 *     circuit (it has fewer than pieces * n coefficients): 5 of the 8 cosets of the extended domain for the reference's circuits;
 *   d_h: pieces x 2^log_n coefficients of h, piece t = coefficients [t n, (t + 1) n).
 * With all E cosets the result equals hm_extended_to_coeff of the divided whole-array evaluation word for word for ANY
 * columns; with fewer it is the polynomial of degree < count * n through the numerator / (X^n - 1) on those cosets -- the same
 * h exactly when the circuit is satisfied.  Asynchronous on `stream`; the workspace (columns x (count + 1) + count arrays of n)
 * belongs to the stream's slot. */
int hm_quotient_by_cosets_bn256_fr_dev(uint64_t program, const void* const* d_coeff_columns, const void* const* d_on_cosets, size_t n_columns,
                                       const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t log_n, const uint64_t omega[4],
                                       const uint64_t* shifts, size_t count, size_t pieces, void* d_h, void* stream);
/* The same in two steps, for a proof split over several GPUs: every device runs hm_quotient_partials on ITS cosets (same
 * arguments; d_partials: count x 2^log_n words, the partial of shifts[c] at c * 2^log_n), the partials travel to one device
 * (2^log_n x 32 B per coset), and hm_quotient_combine turns ALL of them -- d_partials: host array of `count` device pointers in the
 * order of `shifts`, count <= 64 -- into the pieces of h.  hm_quotient_by_cosets is the two on one device. */
int hm_quotient_partials_bn256_fr_dev(uint64_t program, const void* const* d_coeff_columns, const void* const* d_on_cosets, size_t n_columns,
                                      const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t log_n, const uint64_t omega[4],
                                      const uint64_t* shifts, size_t count, void* d_partials, void* stream);
int hm_quotient_combine_bn256_fr_dev(const void* const* d_partials, const uint64_t* shifts, size_t count, uint32_t log_n, size_t pieces, void* d_h,
                                     void* stream);
int hm_graph_destroy(uint64_t handle);
/* The same evaluation with options.  HM_GRAPH_COLUMNS_INTERNAL: every column of the table (short ones included) holds
 * 32 * value mod r instead of value -- the library's internal Montgomery radix is 2^261, so such words need no conversion
 * product when they are loaded (a third of the multiplications of the MerkleSumTree circuit's evaluate_h program are
 * conversions of column loads).  A prover gets its extended-domain columns in that form for nothing: the coset constants
 * of hm_coeff_to_extended_bn256_fr_dev are multiplied into the first NTT pass anyway, so it passes {32, 32 zeta, 32 zeta^2}
 * there (fixed and permutation columns of the proving key: once, at keygen).  PreviousValue on entry, the program's
 * constants and the result written to d_values stay ordinary Fr words.  flags = 0 is hm_graph_evaluate_dev. */
#define HM_GRAPH_COLUMNS_INTERNAL 1
int hm_graph_evaluate_flags_dev(uint64_t handle, const void* const* d_columns, size_t n_columns, const uint64_t* dynamic_constants,
                                size_t n_dynamic, uint32_t log_size, void* d_values, uint32_t flags, void* stream);
/* The same program over `segments` back-to-back blocks of 2^log_segment rows (every column holds segments << log_segment rows;
 * short columns stay periodic in the row index): a rotation wraps INSIDE its block.  One launch for several cosets of the
 * extended domain laid out one after the other per column (hm_coeff_to_cosets_bn256_fr_dev): block c = coset c, rotations
 * unscaled.  segments = 1 is hm_graph_evaluate_flags_dev. */
int hm_graph_evaluate_segments_dev(uint64_t handle, const void* const* d_columns, size_t n_columns, const uint64_t* dynamic_constants,
                                   size_t n_dynamic, uint32_t log_segment, uint32_t segments, void* d_values, uint32_t flags, void* stream);
/* Several circuits of ONE constraint system in one launch: d_values holds PreviousValue on entry and, on return, word for word
 * what `circuits` successive hm_graph_evaluate_segments_dev calls on the same d_values would leave, call c reading circuit c's
 * columns.  Column i of circuit c starts column_strides[i] u32 words times c behind column_bases[i] (the convention of
 * hm_mock_gates_dev); a stride of 0 names a column all circuits share (fixed, permutation, l_0 / l_last / l_active, the coset
 * column, a short periodic column).  Both arrays are host memory; a base must be 16-byte aligned and a stride a multiple of 4
 * words.  log_size, segments and flags as in hm_graph_evaluate_segments_dev; circuits * rows <= 2^32.
 * The program must be linear in PreviousValue the way a Horner fold of gate polynomials is: PreviousValue is read exactly once,
 * as the start of the MulAdd chain that ends in the last calculation; every step of that chain multiplies by the same constant
 * (of the program or of the call) and is read by the next step only.  Its value is then Prev * f^T + G(row); the entry counts T
 * on the program as it was created, raises f to it on the host, and folds acc = acc * f^T + G_c(row) over the circuits on the
 * device, one lane per (circuit, row).  Any other program, circuits == 0, a misaligned base or stride, or counts other than the
 * program's: HM_ERR_BAD_ARG, nothing launched. */
int hm_graph_evaluate_circuits_dev(uint64_t handle, const void* const* column_bases, const uint64_t* column_strides, size_t n_columns,
                                   size_t circuits, const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t log_size, uint32_t segments,
                                   void* d_values, uint32_t flags, void* stream);

/* Several INDEPENDENT proofs of one constraint system in one launch, each with its own per-call constants (the theta, beta, gamma, y
 * of its own transcript): for every b < proofs the call leaves in d_values + b * values_stride (u32 words) what
 * hm_graph_evaluate_segments_dev leaves when it is called with row b of dynamic_constants (host, proofs x n_dynamic x 4 u64) and with
 * column i at column_bases[i] + b * column_strides[i] (u32 words; 0: one column for all proofs).  PreviousValue is read from proof b's
 * own values; nothing is folded across proofs, and ANY program is admitted.  One lane per (proof, row); a rotation wraps inside its
 * segment of its own proof.  Bases and d_values 16-byte aligned, strides multiples of 4 words, proofs * rows <= 2^32.
 * HM_ERR_BAD_ARG, nothing launched: proofs == 0, a values_stride below the rows of one proof (8 words a row) unless proofs == 1, a
 * misaligned base or stride, counts other than the program's. */
int hm_graph_evaluate_proofs_dev(uint64_t handle, const void* const* column_bases, const uint64_t* column_strides, size_t n_columns,
                                 size_t proofs, const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t log_size, uint32_t segments,
                                 void* d_values, uint64_t values_stride, uint32_t flags, void* stream);

/* Inputs and known answer of the benchmark of SURVEY.md §8d, without leaving the device:
 *   hm_fr_random_dev           out[i] uniform in [0, r) (Fr::random): one xoshiro256** stream per element, seeded by
 *                              splitmix64 from (seed, i), 254-bit candidates rejected until below r
 *   hm_fr_affine_sequence_dev  out[i] = a + i * b -- the scalars t_i of the bases P_i = [a + i b]G
 *   hm_fr_dot_bn256_dev        out = sum_i a[i] * b[i] (host, 4 u64; synchronises `stream`) -- sum_i s_i t_i, whose
 *                              multiple of G is the MSM's expected result */
int hm_fr_random_dev(void* d_out, size_t n, uint64_t seed, void* stream);
int hm_fr_affine_sequence_dev(void* d_out, size_t n, const uint64_t a[4], const uint64_t b[4], void* stream);
int hm_fr_dot_bn256_dev(const void* d_a, const void* d_b, size_t n, uint64_t out[4], void* stream);

/* a[i] *= c element-wise (device pointer, in place). */
int hm_fr_scale_dev(void* d_a, size_t n, const uint64_t c[4], void* stream);
/* EvaluationDomain::distribute_powers_zeta on its own: a[i] *= c3[i % 3] (device pointer, in place). */
int hm_fr_distribute_powers_dev(void* d_a, size_t n, const uint64_t c3[12], void* stream);

/* ParamsKZG::setup's G1 work: out[i] = [scalars[i]] * base (fixed-base), affine output.
 * scalars: n x 4 u64 device; out: n x 8 u64 device. */
int hm_g1_fixed_base_mul_dev(const void* d_scalars, size_t n, const uint64_t base_xy[8], void* d_out_xy, void* stream);

/* ---- best_fft over G1: stands in for halo2_proofs::arithmetic::best_fft::<bn256::G1> (g_to_lagrange, ParamsKZG::downsize) */

/* Device form: n = 2^log_n affine points (n x 8 u64 Montgomery, (0,0) = identity -- the layout hm_register_bases reads and
 * hm_g1_fixed_base_mul_dev writes), a[i] <- sum_j [omega^(ij)] a[j] in place, asynchronous on `stream`; then, when `scale`
 * is not NULL, every output is multiplied by it.  omega, scale: Fr Montgomery words as for hm_ntt_bn256_fr_dev; omega a
 * 2^log_n-th root of unity; log_n <= 24.  Working memory is allocated per call, stream-ordered on `stream`. */
int hm_g1_fft_bn256_dev(void* d_points_xy, const uint64_t omega[4], uint32_t log_n, const uint64_t* scale, void* stream);

/* Host form: n x 12 u64 Jacobian (x, y, z) as bn256::G1 lays them out, any z (z == 0: identity), in place; outputs
 * normalised to (x, y, 1) / (0, 0, 0) like hm_msm_bn256_g1_jacobian.  `points_xyz` is written only by the final copy from
 * the device: every error code but HM_ERR_PARTIAL_OUTPUT (that copy itself failed) leaves it exactly as it was. */
int hm_g1_fft_bn256(uint64_t* points_xyz, const uint64_t omega[4], uint32_t log_n, const uint64_t* scale);

/* ---- All KZG openings of a polynomial on its domain (Feist / Khovratovich, "FK20") ---------------------------------------- */

/* f = sum_{j<n} f_j X^j with n = 2^log_n <= 2^23, g[i] = [s^i]G1 the monomial SRS points, omega the 2^log_n-th root of unity of
 * EvaluationDomain (ROOT_OF_UNITY squared 28 - log_n times).  Proof t is the opening of the commitment of f at omega^t:
 * [(f(s) - f(omega^t)) / (s - omega^t)]G1.  All n of them cost one Fr NTT of size 2n, 2n scalar multiplications and two FFTs over
 * G1 (sizes 2n and n).  Points are n x 8 u64 affine Montgomery, (0,0) = identity, as for hm_g1_fft_bn256_dev; device pointers;
 * asynchronous on `stream`; working memory is allocated per call, stream-ordered on `stream`.
 *
 * table: from the first n points of g, the 2n points the other call multiplies into (the G1 FFT of size 2n of g reversed and padded
 *        with identities) -- the SRS alone, built once per size.  d_table_xy: 2n x 8 u64; it may not overlap d_g_xy.
 * open_all: `count` <= 65535 polynomials in coefficient form, back to back at d_coeffs (count x n x 4 u64 Montgomery) ->
 *        count x n proofs at d_proofs_xy, row t of a polynomial its opening at omega^t.  The output may overlap neither input.
 * open_all_timed: the same, and out_part_ms receives the device milliseconds of the LAST polynomial's seven steps (coefficient
 *        arrangement, NTT, load-multiply, the stages of size 2n, truncation, the stages of size n, store); waits for `stream`.
 * HM_ERR_BAD_ARG for a null pointer, log_n > 23, count > 65535 or overlapping input and output. */
int hm_kzg_open_table_bn256_dev(const void* d_g_xy, uint32_t log_n, void* d_table_xy, void* stream);
int hm_kzg_open_all_bn256_dev(const void* d_table_xy, const void* d_coeffs, uint32_t log_n, size_t count, void* d_proofs_xy, void* stream);
int hm_kzg_open_all_timed_bn256_dev(const void* d_table_xy, const void* d_coeffs, uint32_t log_n, size_t count, void* d_proofs_xy,
                                    double out_part_ms[7], void* stream);

/* Ledger openings (one id-bound KZG opening per user), one lane per user: the pairing operands of every user's own check.  User b
 * holds row d_indices[b] of a ledger of 2^log_n rows, the id d_ids[b] (4 u64 Montgomery Fr words), `assets` balances at
 * d_balances[b] (assets x 4 words) and the opening d_openings_xy[b] (8 u64 affine Montgomery words, (0, 0) = the identity) of
 * c_gamma = C_id + sum_p gamma^(p+1) C_p at omega^index, with the value y = id + sum_p gamma^(p+1) balance_p.  gamma, omega (the
 * 2^log_n-th root of unity) and c_gamma are HOST words; c_gamma is the caller's: its words are checked to be canonical, not to lie
 * on the curve.  Output d_g1_xy, n_users x 2 x 8 u64: row 2b is pi_b, row 2b + 1 is -R_b with R_b = c_gamma + [r - y]G +
 * [omega^index]pi_b, canonical affine Montgomery words, (0, 0) for the identity -- the d_g1_xy layout of
 * hm_pairing_check_bn256_dev, so that (pi_b, [s]G2), (-R_b, G2) is check b of one pairing call.  Every addition is the complete one.
 * d_flags[b] = 1 for a user whose opening has a coordinate word >= p or is off the curve, whose id or balance words are >= r, or
 * whose index is >= 2^log_n: that user gets two zero rows -- which WOULD pass a pairing, so the flag decides -- and nothing of it is
 * multiplied; 0 otherwise.  All DEVICE memory but the three word arrays; point and scalar arrays 16-byte aligned, d_indices and d_flags
 * 4-byte.  Asynchronous on `stream`: one launch.  HM_ERR_BAD_ARG, with nothing launched: NULL arguments (d_balances may be NULL when
 * assets is 0), n_users 0 or above 2^20 (the pairing entry's cap), log_n > 28, assets > 2^16, gamma or omega not below r, a word of
 * c_gamma not below p, a buffer that is not aligned. */
int hm_kzg_ledger_pairs_bn256_dev(const void* d_openings_xy, const uint32_t* d_indices, const void* d_ids, const void* d_balances,
                                  const uint64_t gamma[4], const uint64_t omega[4], const uint64_t c_gamma[8], uint32_t log_n,
                                  uint32_t assets, size_t n_users, void* d_g1_xy, uint32_t* d_flags, void* stream);

/* ---- SRS point encodings: ParamsKZG::read / write (compressed G1 and the checked raw format) ---------------------------- */

/* Compressed G1, 32 bytes: canonical x little-endian (Fq::to_bytes), bit 7 of byte 31 = parity of canonical y; the identity is 32
 * zero bytes.  Points: n x 8 u64 affine Montgomery, (0,0) = identity (the hm_register_bases layout).  n <= 2^30 in every form.
 *
 * compress: points -> n x 32 bytes, asynchronous on `stream`.  The points are trusted (no validation).
 * decompress: n x 32 bytes -> points; waits for `stream`.  An entry with x >= p or x^3 + 3 not a square is written as (0,0).
 * check (the checked raw format): every coordinate word < p, and y^2 = x^3 + 3 or the point is (0,0); waits for `stream`.
 * decompress and check return HM_ERR_INVALID_DATA with the smallest bad index in *out_first_invalid, or HM_OK with
 * *out_first_invalid = n. */
int hm_g1_compress_bn256_dev(const void* d_points_xy, size_t n, void* d_out32, void* stream);
int hm_g1_decompress_bn256_dev(const void* d_in32, size_t n, void* d_points_xy, uint64_t* out_first_invalid, void* stream);
int hm_g1_check_bn256_dev(const void* d_points_xy, size_t n, uint64_t* out_first_invalid, void* stream);

/* Host forms of the same, through the library's staging.  The output array is written only by the final copy from the device:
 * every error code but HM_ERR_PARTIAL_OUTPUT (that copy itself failed) leaves it exactly as it was, HM_ERR_INVALID_DATA included. */
int hm_g1_compress_bn256(const uint64_t* points_xy, size_t n, uint8_t* out32);
int hm_g1_decompress_bn256(const uint8_t* in32, size_t n, uint64_t* points_xy, uint64_t* out_first_invalid);
int hm_g1_check_bn256(const uint64_t* points_xy, size_t n, uint64_t* out_first_invalid);

/* ---- Poseidon over BN256 Fr and Merkle (sum) trees --------------------------------------------- */

/* Poseidon as halo2_gadgets::poseidon::primitives::Hash<Fr, Spec, ConstantLength<L>, WIDTH, RATE> with L = RATE (one permutation
 * per hash): state = [m_0 .. m_{RATE-1}, L * 2^64]; r_f / 2 full rounds, r_p partial rounds, r_f / 2 full rounds, each
 * `state += rc[r]; x^5 on every word (full) or on word 0 (partial); state = MDS * state`; digest = state[0].
 * The constants are DATA: hand over Spec::constants() verbatim (round_constants: (r_f + r_p) x width elements, mds: width x width
 * row-major, each 4 x u64 Montgomery).  HM_ERR_BAD_ARG for width other than 3 or 5, rate != width - 1, an odd r_f, r_f + r_p = 0 or
 * above 1024, or a constant >= r.  The handle owns a small device buffer until hm_poseidon_destroy / hm_shutdown. */
int hm_poseidon_create(uint32_t width, uint32_t rate, uint32_t r_f, uint32_t r_p, const uint64_t* round_constants, const uint64_t* mds,
                       uint64_t* out_handle);
int hm_poseidon_destroy(uint64_t handle);
/* n messages of `rate` elements each (n x rate x 4 u64) -> n digests (n x 4 u64).  _dev: asynchronous on `stream`; the host form
 * goes through the library's staging and writes `out` only by its final copy. */
int hm_poseidon_hash_bn256_fr_dev(uint64_t handle, const void* d_msgs, size_t n, void* d_out, void* stream);
int hm_poseidon_hash_bn256_fr(uint64_t handle, const uint64_t* msgs, size_t n, uint64_t* out);
/* Merkle sum tree (the reference's compute_merkle_sum_root): a node is (hash, balance), 2 elements; parent.hash =
 * H(left.hash, left.balance, right.hash, right.balance) with a width-5 spec, parent.balance = left.balance + right.balance mod r.
 * d_nodes receives all 2^(depth+1) - 1 nodes, level by level: the 2^depth leaves first (copied from d_leaves, which may be d_nodes
 * itself), then 2^(depth-1) parents, ... the root last.  depth <= 30; a handle of another width is HM_ERR_BAD_ARG.
 * Host form: root (2 elements) and, unless NULL, all nodes; both are written only after the tree is built. */
int hm_merkle_sum_tree_build_dev(uint64_t handle, const void* d_leaves, uint32_t depth, void* d_nodes, void* stream);
int hm_merkle_sum_tree_build(uint64_t handle, const uint64_t* leaves, uint32_t depth, uint64_t* root, uint64_t* nodes_or_null);
/* The plain tree of a width-3 spec (merkle_v3): one element per node, parent = H(left, right); same node order. */
int hm_merkle_tree_build_dev(uint64_t handle, const void* d_leaves, uint32_t depth, void* d_nodes, void* stream);
/* Sibling nodes of m leaves, bottom up: d_out[(p * depth + l) * words_per_node ..] = node ((d_indices[p] >> l) ^ 1) of level l.
 * words_per_node = elements per node (2 sum tree, 1 plain tree); d_indices is DEVICE memory; an index >= 2^depth yields zeros. */
int hm_merkle_paths_dev(const void* d_nodes, uint32_t depth, uint32_t words_per_node, const uint64_t* d_indices, size_t m, void* d_out,
                        void* stream);
/* A built tree updated in place, so that it equals the tree built from the changed leaves.  d_nodes: all 2^(depth+1) - 1 nodes as
 * the build entries write them; d_indices m u64 and d_new_leaves m leaves (2 elements each for the sum tree, 1 for the plain tree),
 * both DEVICE memory.  The result is as if the m entries were applied one after another in array order: of a repeated index the last
 * entry wins; an index >= 2^depth is dropped.  Only the nodes on the paths of the surviving entries are written, one hash per
 * distinct touched node.  Asynchronous on `stream`, nothing comes back to the host; scratch is the library's, stream-ordered.
 * d_counts_or_null: depth + 1 u32 in DEVICE memory: the surviving entries, then the nodes hashed at levels 1 .. depth.
 * HM_ERR_BAD_ARG: NULL with m > 0, depth 0 or above 30, m > 2^31, a handle of another width, a pointer not 16-byte aligned (8 for
 * d_indices, 4 for the counts), d_new_leaves overlapping the nodes.  m = 0 writes nothing (zeros to the counts).  There is no host
 * form: it would upload the whole tree to save part of building it. */
int hm_merkle_sum_tree_update_dev(uint64_t handle, uint32_t depth, void* d_nodes, const uint64_t* d_indices, const void* d_new_leaves,
                                  size_t m, uint32_t* d_counts_or_null, void* stream);
int hm_merkle_tree_update_dev(uint64_t handle, uint32_t depth, void* d_nodes, const uint64_t* d_indices, const void* d_new_leaves,
                              size_t m, uint32_t* d_counts_or_null, void* stream);
/* The roots of m paths, one lane per path and depth hashes in sequence: leaves m x E elements, siblings m x depth x E elements as
 * hm_merkle_paths_dev writes them, indices m u64 (bit l = the path's node is the RIGHT child at level l; higher bits are ignored)
 * -> roots m x E elements.  The handle's width selects E: 5 -> 2, (hash, balance) with the balances summed mod r along the path
 * (compute_merkle_sum_root); 3 -> 1.  Comparing with an expected root is the caller's business.  0 < depth <= 30, m <= 2^31; _dev:
 * 16-byte aligned pointers (8 for d_indices), asynchronous on `stream`; the host form goes through the library's staging and
 * writes `roots` only by its final copy. */
int hm_merkle_roots_bn256_dev(uint64_t handle, uint32_t depth, size_t m, const void* d_leaves, const void* d_siblings,
                              const uint64_t* d_indices, void* d_roots, void* stream);
int hm_merkle_roots_bn256(uint64_t handle, uint32_t depth, size_t m, const uint64_t* leaves, const uint64_t* siblings,
                          const uint64_t* indices, uint64_t* roots);
/* The witness of the reference's MerkleSumTree circuit (one inclusion path per user), filled on the GPU: the advice columns as
 * MerkleSumTreeChip::synthesize assigns them, the Pow5 chip's trace of every Poseidon round among them.
 * layout: the rows and columns the call below fills for a spec with r_f / r_p rounds (r_p even); needs no device.  out_regions, unless
 * NULL, receives 4 numbers: rows of a "permute state" region, rows of one level, the row of the less-than region, the first row
 * of the constants.  HM_ERR_BAD_ARG for depth 0 or above 32, an odd r_f or r_p, log_n above 24, or rows_used > 2^log_n - 6.
 * witness: m users; d_leaves m x 2 elements (hash, balance), d_siblings m x depth x 2 elements as hm_merkle_paths_dev writes them,
 * d_indices m u64 (bit l = the path's node is the RIGHT child at level l; higher bits are ignored), assets_sum one element in HOST
 * memory; all elements canonical.  d_nodes_or_null: the tree hm_merkle_sum_tree_build_dev built (depth <= 30), from which the
 * path's nodes are read; NULL: they are hashed from the siblings, one chain per user.  d_advice: m x n_advice x 2^log_n elements
 * (column c of user u is contiguous), every word of which is written (unassigned cells and the last rows are zero: blinding is the
 * prover's business); d_instance: m x 4 elements (leaf hash, leaf balance, root, assets).  Nothing is judged: a sum above the
 * assets gives an unsatisfied witness.  Asynchronous on `stream`.  Arguments are checked before anything is launched.  Every device
 * pointer must be 16-byte aligned (elements are moved as two 16-byte halves; d_indices: 8), and one that is not is refused with
 * HM_ERR_BAD_ARG like every other bad argument; d_nodes must hold all 2^(depth+1) - 1 nodes of `depth`.
 * Host form: m * n_advice * 2^log_n * 32 bytes <= 256 MiB; outputs are written only by the final copies. */
int hm_merkle_sum_witness_layout(uint32_t r_f, uint32_t r_p, uint32_t depth, uint32_t log_n, uint32_t* out_rows_used,
                                 uint32_t* out_n_advice, uint32_t* out_regions);
int hm_merkle_sum_witness_bn256_dev(uint64_t handle, uint32_t depth, uint32_t log_n, size_t m, const void* d_leaves,
                                    const void* d_siblings, const uint64_t* d_indices, const uint64_t* assets_sum,
                                    const void* d_nodes_or_null, void* d_advice, void* d_instance, void* stream);
int hm_merkle_sum_witness_bn256(uint64_t handle, uint32_t depth, uint32_t log_n, size_t m, const uint64_t* leaves,
                                const uint64_t* siblings, const uint64_t* indices, const uint64_t* assets_sum, uint64_t* advice,
                                uint64_t* instance);

/* The witnesses of the reference's two other circuits, with the same conventions as the sum tree's above.
 * MerkleTreeV3 (width-3 spec): d_leaves m elements, d_siblings m x depth elements as hm_merkle_paths_dev writes them with one
 * word per node, d_nodes_or_null the tree of hm_merkle_tree_build_dev; d_advice m x 7 x 2^log_n elements (a b c | state[3] |
 * partial_sbox), d_instance m x 2 (leaf, root).  out_regions, unless NULL, receives 3 numbers: rows of a "permute state" region,
 * rows of one level, the first row of the constants.
 * Poseidon circuit (width-5 spec): d_msgs m x 4 elements; d_advice m x 6 x 2^log_n (state[5] | partial_sbox), d_instance m x 1
 * (the digest).  out_regions: rows of "permute state", rows before the constants, the first row of the constants.
 * HM_ERR_BAD_ARG: a handle of the wrong width, depth 0 or above 32, a tree pointer with depth above 30, an odd r_f or r_p, log_n
 * above 24, rows_used > 2^log_n - 6, a device pointer that is not 16-byte aligned (d_indices: 8), m == 0, more than 2^31 hashes;
 * the host forms: more than 256 MiB of columns.  Nothing is written or launched in those cases. */
int hm_merkle_witness_layout(uint32_t r_f, uint32_t r_p, uint32_t depth, uint32_t log_n, uint32_t* out_rows_used, uint32_t* out_n_advice,
                             uint32_t* out_regions);
int hm_merkle_witness_bn256_dev(uint64_t handle, uint32_t depth, uint32_t log_n, size_t m, const void* d_leaves, const void* d_siblings,
                                const uint64_t* d_indices, const void* d_nodes_or_null, void* d_advice, void* d_instance, void* stream);
int hm_merkle_witness_bn256(uint64_t handle, uint32_t depth, uint32_t log_n, size_t m, const uint64_t* leaves, const uint64_t* siblings,
                            const uint64_t* indices, uint64_t* advice, uint64_t* instance);
int hm_poseidon_witness_layout(uint32_t r_f, uint32_t r_p, uint32_t log_n, uint32_t* out_rows_used, uint32_t* out_n_advice,
                               uint32_t* out_regions);
int hm_poseidon_witness_bn256_dev(uint64_t handle, uint32_t log_n, size_t m, const void* d_msgs, void* d_advice, void* d_instance,
                                  void* stream);
int hm_poseidon_witness_bn256(uint64_t handle, uint32_t log_n, size_t m, const uint64_t* msgs, uint64_t* advice, uint64_t* instance);

/* The witness of the range-check circuit (the reference's OverflowChipV2): advice column 0 holds the values, columns 1 .. acc_cols
 * their limbs of max_bits bits, most significant first, so that sum limb_i * 2^(max_bits * (acc_cols - 1 - i)) = value whenever the
 * value is below 2^(max_bits * acc_cols).
 * layout: needs no device; *out_n_advice = 1 + acc_cols, *out_table_rows = 2^max_bits, the rows of the fixed range column.
 * witness: m circuits of `rows` values each; d_values m x rows canonical elements; d_advice m x (1 + acc_cols) x 2^log_n elements
 * (column c of circuit u is contiguous), every word of which is written: rows >= `rows` are zero (blinding is the prover's business).
 * The limbs are the low max_bits * acc_cols bits of the value; nothing is judged: a larger value gives a witness that fails the gate,
 * and d_over_or_null, unless NULL, receives per circuit the number of such values (m u32, set by every call).  Asynchronous on
 * `stream`; no stream-ordered memory of the library's is used.
 * HM_ERR_BAD_ARG, before anything is written or launched: a NULL pointer other than d_over_or_null, max_bits outside 1 .. 16,
 * acc_cols = 0, max_bits * acc_cols > 253, log_n above 24, rows = 0, max(rows, 2^max_bits) > 2^log_n - 6, m = 0, m * 2^log_n > 2^31,
 * a device pointer that is not 16-byte aligned (d_over: 4), d_values overlapping d_advice; the host form: more than 256 MiB of columns.
 * Host form: outputs are written only by the final copies. */
int hm_range_witness_layout(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, uint32_t rows, uint32_t* out_n_advice,
                            uint32_t* out_table_rows);
int hm_range_witness_bn256_fr_dev(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const void* d_values,
                                  void* d_advice, uint32_t* d_over_or_null, void* stream);
int hm_range_witness_bn256_fr(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint64_t* values,
                              uint64_t* advice, uint32_t* over_or_null);

/* The witness of the sorted-column circuit (this project's own: "the ids of this committed column are pairwise distinct"): advice
 * column 0 holds the ids, columns 1 .. acc_cols on rows 0 .. rows - 2 the limbs of the gap id[i+1] - id[i] - 1 mod r, max_bits bits
 * each, most significant first, so that the gap equals sum limb_j * 2^(max_bits * (acc_cols - 1 - j)) whenever it is below
 * 2^(max_bits * acc_cols); the limbs of row rows - 1 and of every row behind it are zero.
 * layout: needs no device; *out_n_advice = 1 + acc_cols, *out_table_rows = 2^max_bits, the rows of the fixed range column.
 * witness: m circuits of `rows` ids each; d_ids m x rows canonical elements; d_advice m x (1 + acc_cols) x 2^log_n elements (column c
 * of circuit u is contiguous), every word of which is written.  The limbs are the low max_bits * acc_cols bits of the gap; nothing is
 * judged: ids that are not ascending, equal or too far apart give a witness that fails the gate, and d_over_or_null, unless NULL,
 * receives per circuit the number of such rows (m u32, set by every call).  Asynchronous on `stream`; no stream-ordered memory of the
 * library's is used.
 * HM_ERR_BAD_ARG, before anything is written or launched: what hm_range_witness_* refuse, and max_bits * acc_cols + log_n > 253 (with
 * it no two ids of a column whose gaps are all in range agree mod r). */
int hm_sorted_witness_layout(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, uint32_t rows, uint32_t* out_n_advice,
                             uint32_t* out_table_rows);
int hm_sorted_witness_bn256_fr_dev(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const void* d_ids,
                                   void* d_advice, uint32_t* d_over_or_null, void* stream);
int hm_sorted_witness_bn256_fr(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint64_t* ids,
                               uint64_t* advice, uint32_t* over_or_null);
/* The order that brings a column into the sorted-column circuit's: d_perm[0 .. n) receives the rows of the n canonical Montgomery
 * elements of d_values, as 64-bit integers, sorted by the elements' canonical integers, equal elements by ascending row -- a
 * function of the input alone.  A bitonic network over (key, row) records of 9 words, the same launches whatever the values;
 * asynchronous on `stream`, with stream-ordered scratch of the library's (36 bytes for each of the next power of two of n).
 * HM_ERR_BAD_ARG, before anything is launched: NULL, n = 0 or above 2^26, d_values not 16-byte or d_perm not 8-byte aligned, the two
 * overlapping. */
int hm_fr_argsort_bn256_dev(const void* d_values, size_t n, uint64_t* d_perm, void* stream);

/* The witness of the accumulator circuit (the reference's SafeAccumulator): a running total of acc_cols limbs of max_bits bits, most
 * significant first, W = max_bits * acc_cols <= 64 bits in all.  Advice column 0 holds the added values, column 1 the inverse of the
 * top limb (0 when that limb is 0), columns 2 .. 1 + acc_cols the binary carries, columns 2 + acc_cols .. 1 + 2 acc_cols the limbs.
 * Row 0 holds the initial limbs as given (every other cell of it zero); row r, 1 <= r <= rows, the value r and the state after adding
 * it: S_r = (S_(r-1) + (value_r mod 2^W)) mod 2^W, S_0 the initial limbs read as one integer mod 2^W; carry[acc_cols - 1] =
 * (limb + value >= 2^max_bits), carry[i] = (limb_i of S_(r-1) + carry[i + 1] >= 2^max_bits), carry[0] = 0.
 * layout: needs no device; *out_n_advice = 2 + 2 acc_cols, *out_used_rows = rows + 1.
 * witness: m circuits of `rows` values each; d_values m x rows canonical elements; d_initial m x acc_cols plain limb integers;
 * d_advice m x (2 + 2 acc_cols) x 2^log_n elements (column c of circuit u is contiguous), every word of which is written: rows above
 * `rows` are zero; d_finals m x acc_cols: the plain limbs of S_rows, which are the circuit's instance.  Nothing is judged: a value at
 * or above 2^max_bits, an initial limb at or above 2^max_bits or a total that reaches the top limb gives a witness that fails its
 * gates; d_over_or_null, m counters in DEVICE memory set by every call, counts per circuit the rows r >= 1 whose value is at or above
 * 2^max_bits or whose top limb is not zero, plus 1 when an initial limb is at or above 2^max_bits or the initial top limb is not zero.
 * Asynchronous on `stream`: four launches with stream-ordered scratch of the library's; no kernel waits for another block.
 * HM_ERR_BAD_ARG, before anything is launched: NULL (d_over excepted), max_bits outside 1 .. 4, acc_cols < 2, max_bits * acc_cols > 64,
 * log_n above 24, rows = 0, rows + 1 > 2^log_n - 6, m = 0 or above 65535, m * 2^log_n > 2^31, a device pointer that is not aligned
 * (d_values, d_advice: 16; d_initial, d_finals: 8; d_over: 4), an output overlapping an input; the host form: more than 256 MiB of
 * columns.  Host form: outputs are written only by the final copies. */
int hm_accumulator_witness_layout(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, uint32_t rows, uint32_t* out_n_advice,
                                  uint32_t* out_used_rows);
int hm_accumulator_witness_bn256_fr_dev(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const void* d_values,
                                        const uint64_t* d_initial, void* d_advice, uint64_t* d_finals, uint32_t* d_over_or_null,
                                        void* stream);
int hm_accumulator_witness_bn256_fr(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const uint64_t* values,
                                    const uint64_t* initial, uint64_t* advice, uint64_t* finals, uint32_t* over_or_null);
/* The device form, and out_part_ms receives the device milliseconds of its four launches (the block totals, their scan, the rows, the
 * counters; the last is 0 without d_over); waits for `stream`.  For tools/accumulator_witness_time.py. */
int hm_accumulator_witness_timed_bn256_fr_dev(uint32_t max_bits, uint32_t acc_cols, uint32_t log_n, size_t m, uint32_t rows, const void* d_values,
                                              const uint64_t* d_initial, void* d_advice, uint64_t* d_finals, uint32_t* d_over_or_null,
                                              void* stream, double out_part_ms[4]);

/* keygen's permutation argument (permutation::keygen::Assembly) on the device.  A cell id is j * 2^k + i: column j of the
 * `columns` equality-enabled columns, row i; columns * 2^k <= 2^32.
 * assemble: d_copies holds m copy constraints as pairs of cell ids (DEVICE memory, 8-byte aligned).  d_sigma_cells receives
 * columns * 2^k ids, the permutation as cells: a cell no copy names maps to itself; the members of every class of cells joined
 * by copies, by ascending id, each map to the next one and the last to the first.  The result depends on the set of copies
 * alone, not on their order or on scheduling.  m = 0 gives the identity.  A pair with an id >= columns * 2^k is dropped, and counted
 * in *d_dropped_or_null (one u32 in DEVICE memory, set by every call) unless that is NULL.
 * columns: d_out[c] = delta^j' * omega^i' for d_sigma_cells[c] = j' * 2^k + i', c < columns * 2^k: the `columns` sigma columns
 * in Lagrange form, back to back (an id out of range gives zero); omega and delta are 4 Montgomery words each in HOST memory.
 * Both are asynchronous on `stream`, a fixed chain of launches with stream-ordered scratch of the library's; nothing comes back
 * to the host.  HM_ERR_BAD_ARG, before anything is launched: NULL with work to do, columns = 0, columns * 2^k > 2^32, 2 m > 2^31,
 * a pointer that is not aligned (d_copies 8, d_out 16, the others 4), an output overlapping its input. */
int hm_permutation_assemble_dev(const uint32_t* d_copies, size_t m, uint32_t columns, uint32_t k, uint32_t* d_sigma_cells,
                                uint32_t* d_dropped_or_null, void* stream);
int hm_permutation_columns_bn256_fr_dev(const uint32_t* d_sigma_cells, uint32_t columns, uint32_t k, const uint64_t omega[4],
                                        const uint64_t delta[4], void* d_out, void* stream);

/* MockProver::verify for a BATCH of witnesses on the device: does every user's witness satisfy the constraint system?  Three passes
 * over one batched column table, the program's table (fixed, then advice, then instance) with m users behind every entry: column i
 * starts at column_bases[i] (DEVICE memory, 16-byte aligned), user u's copy lies column_strides[i] u32 words further per user (a
 * multiple of 4; 0: one column shared by all users, i.e. a fixed column), and holds column_rows[i] <= 2^k elements of 4 Montgomery
 * words -- a cell above them reads as zero, so an instance column is given as it is, never padded.  The three arrays are HOST memory.
 * gates: the hm_graph_create program `graph` runs on one lane per (user, row < usable_rows); a rotation wraps modulo 2^k inside the
 *   user's own columns; PreviousValue is zero; a lane whose value is not zero is a failure.  With d_lanes_or_null (DEVICE memory,
 *   n_lanes records of an earlier call) only those lanes run; a record naming a user or row outside the batch is skipped.
 * copies: d_copies (DEVICE memory, 8-byte aligned) holds n_copies pairs of cell ids as hm_permutation_assemble_dev takes them,
 *   permutation column j being entry permutation_columns[j] (HOST memory) of the table; one lane per (user, copy) compares the two
 *   cells' words.  A copy between two shared columns is checked for user 0 only; a pair naming a column >= n_permutation is skipped.
 * lookup: `graph` is the input expression of one lookup; d_table_values holds 2^k elements (DEVICE memory, 16-byte aligned) whose
 *   first usable_rows are the table.  They are brought to canonical integers and sorted once per call; a lane fails when its
 *   value's canonical integer is not among them.  user_base is added to the user index of every record and flag of the call.
 * Failures: a record is user << 32 | row (gates, lookup) or user << 32 | copy index.  Every wave adds its failures to *d_counter (one
 * u64, DEVICE memory) with one atomic and writes the records whose slot is below cap into d_records (cap u64, DEVICE memory); the
 * counter keeps counting past cap, so it is exact.  The counter is the caller's: zero it before the first call; calls add to it and
 * append behind the records already there.  d_user_flags[user] (DEVICE bytes, one per user) is set to 1 for a user with a failure and
 * otherwise left alone.  No other device memory of the caller's is written.  The launches are asynchronous on `stream`; the call then
 * waits for the stream to read the counter back into *out_total.
 * HM_ERR_BAD_ARG, with nothing written or launched: NULL arguments, no or more than 256 columns, k > 30, m == 0, cap == 0, a column
 * with more than 2^k rows, a pointer or stride that is not aligned, usable_rows 0 or above 2^k, m * usable_rows > 2^32, a lane list that
 * is empty or not 8-byte aligned, a permutation column outside the table, n_copies == 0, a program built for another number of columns
 * or per-call constants.  HM_ERR_NOT_FOUND: an unknown program handle. */
int hm_mock_gates_dev(uint64_t graph, const void* const* column_bases, const uint64_t* column_strides, const uint32_t* column_rows,
                      size_t n_columns, const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t k, uint32_t usable_rows, size_t m,
                      const uint64_t* d_lanes_or_null, size_t n_lanes, uint64_t* d_records, size_t cap, uint64_t* d_counter,
                      uint8_t* d_user_flags, uint64_t* out_total, void* stream);
int hm_mock_copies_dev(const void* const* column_bases, const uint64_t* column_strides, const uint32_t* column_rows, size_t n_columns,
                       const uint32_t* permutation_columns, size_t n_permutation, const uint32_t* d_copies, size_t n_copies, uint32_t k,
                       size_t m, uint64_t* d_records, size_t cap, uint64_t* d_counter, uint8_t* d_user_flags, uint64_t* out_total,
                       void* stream);
int hm_mock_lookup_dev(uint64_t graph, const void* const* column_bases, const uint64_t* column_strides, const uint32_t* column_rows,
                       size_t n_columns, const uint64_t* dynamic_constants, size_t n_dynamic, uint32_t k, uint32_t usable_rows, size_t m,
                       uint32_t user_base, const void* d_table_values, uint64_t* d_records, size_t cap, uint64_t* d_counter,
                       uint8_t* d_user_flags, uint64_t* out_total, void* stream);

/* ---- a batch of proofs: what halo2_proofs::plonk::BatchVerifier does per proof around its one pairing ------------------------------
 *
 * read: n_proofs proofs of `slots` 32-byte slots each lie one behind the other in d_proofs (DEVICE memory, 16-byte aligned).  What a
 * slot holds is the same for every proof of one constraint system and stands in d_slot_table (DEVICE memory, one u32 per slot):
 * bit 31 set for a compressed G1 point, clear for a scalar; bits 0 .. 29 the slot's index among the proof's points, or among its
 * scalars; bit 30, on a point, sends it to the tail.  One lane per (proof, slot):
 *   a point is decompressed as by hm_g1_decompress_bn256_dev, into 8 u64 affine Montgomery words (the hm_register_bases layout): at row
 *     b * own_points + index of d_points_xy, or with bit 30 at row b of d_tail_xy; the 32 canonical bytes of its y go to row
 *     b * points + index of d_y_bytes (the transcript absorbs x, which the proof holds, then y);
 *   a scalar must be below r and is written as 4 Montgomery words to row b * scalars + index of d_scalars.
 * A slot that cannot be read -- x >= p, x^3 + 3 not a square, the 32 zero bytes of the identity, a scalar >= r, a table entry whose
 * index lies outside its array (index >= points, >= own_points without bit 30, >= scalars) -- sets d_bad[b] (one u32 per proof, zeroed
 * by the caller) to 1; its outputs are zeros, or for a table entry outside its array are left alone.  Asynchronous on `stream`.
 * HM_ERR_BAD_ARG, with nothing launched: NULL arguments, n_proofs 0 or above 2^24, slots 0 or above 2^16, points + scalars != slots,
 * own_points > points, a buffer that is not aligned.
 *
 * column sum: d_out[c] = the sum mod r of rows lo .. hi - 1 of column c of d_rows, an (n_rows, columns) array of Montgomery Fr words
 * (DEVICE memory, 16-byte aligned; d_out: columns x 4 u64): the contributions of the proofs lo .. hi - 1 to the points all proofs
 * share.  lo == hi gives zeros.  Asynchronous on `stream`.  HM_ERR_BAD_ARG, with nothing launched: NULL arguments, columns 0 or above
 * 2^16, lo > hi, hi > n_rows, n_rows > 2^24, a buffer that is not aligned. */
int hm_verify_read_proofs_dev(const void* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots, uint32_t own_points,
                              uint32_t points, uint32_t scalars, void* d_points_xy, void* d_tail_xy, void* d_y_bytes, void* d_scalars,
                              uint32_t* d_bad, void* stream);
int hm_verify_column_sum_dev(const void* d_rows, size_t n_rows, uint32_t columns, size_t lo, size_t hi, void* d_out, void* stream);
/* terms: one lane per proof computes r_b x the scalar of every point of the proof's opening check, from d_records (n_proofs x 9
 * elements: theta, beta, gamma, y, x, the multiopen's y', v, u, and the weight r_b), d_scalars (the evaluations, as the read call left
 * them) and d_instance (the instance values, column after column, every column padded to the plan's row count) -- all 4 Montgomery
 * words per element, DEVICE memory.  `plan` (HOST memory, n_plan_words u32; csrc/verify_terms.inc states its layout) is built once per
 * constraint system: where a (column, rotation) of the program stands in the proof's value row, the instance queries, the rotation sets
 * of the multiopen taken on rotations, the constants.  It is checked word by word -- every index it holds must lie inside its array --
 * and uploaded with the call.  `graph` is the hm_graph_create program of the gate, permutation and lookup expressions folded in y,
 * undivided, lowered from the constraint system alone; n_columns / n_dynamic are its own counts (its per-call constants must be beta,
 * gamma, theta, y).  The lane computes x^n, l0, l_last, l_active and the instance columns' evaluations at x, runs the program on its
 * value row (PreviousValue zero), divides by x^n - 1, and per rotation set the multiopen's scalars.
 * Output (DEVICE memory, written for every proof): d_own, n_proofs x own points x 4 words, the proof's own points in the proof's
 * order ([h] last, the h pieces weighted by the powers of x^n); d_shared, n_proofs x shared points x 4, its row of the shared points'
 * array; d_h2_r / d_h2_l, n_proofs x 4 each: r_b u and r_b, the weights of [h'] in the two sums.  A proof whose d_bad[b] is set on
 * entry, or that would divide by zero (x^n = 1, x = 0, u on a point of the opening), gets all-zero rows and d_bad[b] = 1: a zero is
 * never inverted into a fault.  Asynchronous on `stream`.
 * HM_ERR_BAD_ARG, with nothing launched: NULL arguments, n_proofs 0 or above 2^20, a plan that fails its check -- among the reasons an
 * instance column longer than 64 rows and more than 256 value slots --, column or constant counts that are not the program's, an
 * unknown program handle. */
int hm_verify_terms_dev(uint64_t graph, const uint32_t* plan, size_t n_plan_words, size_t n_columns, size_t n_dynamic, size_t n_proofs,
                        const void* d_records, const void* d_scalars, const void* d_instance, uint32_t* d_bad, void* d_own, void* d_shared,
                        void* d_h2_r, void* d_h2_l, void* stream);
/* terms of multi-circuit proofs (create_proof_multi): as hm_verify_terms_dev, for n_proofs proofs of `circuits` circuits each, 1 <=
 * circuits <= 64.  One WAVEFRONT per proof, lane c is circuit c: a lane computes x^n, the Lagrange values and the instance evaluations
 * of its own circuit, runs the SAME program on its own value row -- its circuit's evaluations, the shared ones, its instance
 * evaluations -- and the proof's numerator sum_c y^(E (circuits - 1 - c)) N_c (E expressions per circuit) and the sum of
 * coeff x r_eval meet by cross-lane moves inside the wave: no atomics, nothing leaves the wavefront.  Lanes at and above `circuits`
 * take no part.  `plan` is the multi plan (csrc/verify_terms.inc, second half): the single-circuit plan of one lane, and where a lane
 * finds its circuit's scalars and own rows in the proof; it is checked word by word, the per-circuit strides for the LAST circuit.
 * d_records: n_proofs x 9 elements as above; d_scalars: n_proofs x (the proof's scalars) in the proof's order; d_instance: n_proofs x
 * circuits rows, each as hm_verify_terms_dev takes one.  Output as above, per PROOF: d_own n_proofs x (the proof's own points) x 4
 * words in the proof's point order, d_shared, d_h2_r, d_h2_l.  If any lane of a proof would divide by zero, or d_bad[b] is set on
 * entry, the proof gets all-zero rows and d_bad[b] = 1.  At circuits = 1 the words are hm_verify_terms_dev's.  Asynchronous on `stream`.
 * HM_ERR_BAD_ARG, with nothing launched: NULL arguments, circuits 0 or above 64, n_proofs 0 or above 2^16, a buffer that is not
 * 4-byte aligned, a plan that fails its check or was built for another `circuits`, an unknown program handle. */
int hm_verify_terms_multi_dev(uint64_t graph, const uint32_t* plan, size_t n_plan_words, size_t n_columns, size_t n_dynamic, size_t n_proofs,
                              uint32_t circuits, const void* d_records, const void* d_scalars, const void* d_instance, uint32_t* d_bad,
                              void* d_own, void* d_shared, void* d_h2_r, void* d_h2_l, void* stream);
/* terms of proofs that end in the GWC multiopen (ProverGWC / VerifierGWC: one witness point W_i per distinct query point z_i, the
 * check e(sum_i u^i W_i, [s]G2) = e(sum_i u^i z_i W_i + sum_i u^i sum_j v^j C_ij - (sum_i u^i sum_j v^j e_ij) G, G2)): as
 * hm_verify_terms_dev, one lane per proof, the same `graph`, the same phase before the multiopen.  d_records: n_proofs x 8 elements
 * -- theta, beta, gamma, y, x, the multiopen's v, u, and the weight r_b: what hm_verify_transcript_dev / _evm_dev leave with
 * record_elems = 8 and a schedule of seven challenges.  `plan` is a GWC plan (csrc/verify_terms.inc, at vg_plan_problem): the header,
 * column map, instance queries and constants of hm_verify_terms_dev's plan, and the q <= 32 point groups -- the constant omega^rot
 * of z_i = x omega^rot, the own row of W_i, the members' targets and evaluation slots -- in place of the rotation sets.  It is checked
 * word by word and uploaded with the call.  The lane computes r_b u^i v^j for member j of group i and ADDS it to the member's row (a
 * commitment opened at several points is a member of several groups; the h commitment is expanded over its pieces by the powers
 * of x^n), sums the generator's scalar, and has no inversion besides 1 / (x^n - 1) and those of the Lagrange values.
 * Output (DEVICE memory, written for every proof): d_own, n_proofs x own points x 4 words in the proof's order -- every point of a
 * GWC proof is an own point, W_i on its row with r_b u^i z_i --; d_shared, n_proofs x shared points x 4, the generator last with
 * -r_b sum u^i v^j e_ij; d_w_left, n_proofs x q x 4: r_b u^i, the scalars of the W_i in the left sum.  A proof whose d_bad[b] is
 * set on entry, or with x^n = 1 or x = 0, gets all-zero rows, d_w_left included, and d_bad[b] = 1.  Asynchronous on `stream`.
 * HM_ERR_BAD_ARG, with nothing launched: as hm_verify_terms_dev, the plan's reasons among them more than 32 point groups. */
int hm_verify_terms_gwc_dev(uint64_t graph, const uint32_t* plan, size_t n_plan_words, size_t n_columns, size_t n_dynamic, size_t n_proofs,
                            const void* d_records, const void* d_scalars, const void* d_instance, uint32_t* d_bad, void* d_own, void* d_shared,
                            void* d_w_left, void* stream);
/* per-proof sums: the two G1 points of every proof's OWN opening check, one workgroup per proof, all proofs in one launch -- what a
 * verdict per proof needs where the MSMs above sum over proofs.  d_bases_xy: (n_proofs * own_points + shared_points + n_proofs) x 8
 * u64, affine Montgomery words, (0, 0) = the identity: the own points of every proof as hm_verify_read_proofs_dev left them, then the
 * points all proofs share, then every proof's tail point [h'].  d_own (n_proofs * own_points x 4 words), d_shared (n_proofs x
 * shared_points x 4), d_h2_r, d_h2_l (n_proofs x 4 each): the Montgomery Fr words hm_verify_terms_dev wrote.  d_bad: n_proofs u32,
 * read only.  Output d_pairs_xy, n_proofs x 2 x 8 u64: row 2b is L_b = h2_l[b] [h']_b, row 2b + 1 is -R_b with
 * R_b = sum_j own[b, j] P[b, j] + sum_k shared[b, k] S_k + h2_r[b] [h']_b, both canonical affine Montgomery words, (0, 0) for the
 * identity -- the d_g1_xy layout of hm_pairing_check_bn256_dev, so that (L_b, [s]G2), (-R_b, G2) is check b of one pairing call.
 * Every addition is the complete one: repeated bases, opposite terms, identity bases and zero scalars give the group's answer.  A
 * proof whose d_bad[b] is set gets two zero rows and nothing of it is multiplied.  All DEVICE memory, 16-byte aligned, d_bad 4-byte.
 * Asynchronous on `stream`: one launch.  HM_ERR_BAD_ARG, with nothing launched: NULL arguments, n_proofs 0 or above 2^20 (the pairing
 * entry's cap), own_points + shared_points 0 or above 2^16 (either may be 0 alone), a buffer that is not aligned. */
int hm_verify_proof_sums_dev(const void* d_bases_xy, size_t n_proofs, uint32_t own_points, uint32_t shared_points, const void* d_own,
                             const void* d_shared, const void* d_h2_r, const void* d_h2_l, const uint32_t* d_bad, void* d_pairs_xy,
                             void* stream);
/* Blake2b-512 (RFC 7693, 64-byte digest, no key), one lane per message: message i is the d_lens[i] bytes at d_msgs + i * stride
 * (DEVICE memory, any alignment; d_lens: n u32, DEVICE memory), personal16 the 16 personalisation bytes (HOST memory, read before the
 * call returns) or NULL for none; d_out: n x 64 digest bytes (DEVICE memory, 4-byte aligned).  The lengths lie on the device, so the
 * call cannot refuse one: a message whose length is above `stride` gets 64 zero bytes and nothing of it is read.  Asynchronous on
 * `stream`.  HM_ERR_BAD_ARG, with nothing launched: NULL arguments (personal16 excepted), n 0 or above 2^24, stride 0 or above
 * 2^32 - 1, d_lens or d_out not 4-byte aligned.
 *
 * transcript: one lane per proof runs the proof's Blake2b transcript (personalisation "Halo2-Transcript"; every absorption behind
 * a prefix byte: 0 a squeeze, 1 a point, 2 a scalar) and leaves its challenges where hm_verify_terms_dev reads them.  d_proofs,
 * d_slot_table, slots and points are those of hm_verify_read_proofs_dev, d_y_bytes what that call wrote.  Proof b first absorbs
 * d_preamble_counts[b] scalars from row b of d_preamble (n_proofs x preamble_stride x 32 canonical little-endian bytes: the digest
 * of the verifying key, then the instance values; the counts may differ from proof to proof), then walks `schedule` (HOST memory,
 * n_schedule_pairs pairs of u32: absorb a slots, then squeeze s challenges) over its slots in order: a point slot absorbs the
 * proof's x bytes with bit 7 of byte 31 cleared and the 32 y bytes of that point, a scalar slot its 32 bytes.  A squeeze absorbs the
 * prefix byte into the running state and finalises a COPY of it; the 64 digest bytes, a little-endian integer, are reduced mod r.
 * Challenge j goes to element j of row b of d_records (n_proofs x record_elems x 4 Montgomery words); the elements behind the
 * schedule's challenges are left alone (the caller's r_b).  A proof whose d_bad_in_out[b] is set on entry is not hashed and gets zero
 * challenges; a preamble count above preamble_stride, or a point slot whose table index is not below `points`, sets d_bad_in_out[b]
 * with zero challenges, and nothing is read outside the arrays.  All DEVICE memory but the schedule; d_proofs, d_y_bytes,
 * d_preamble, d_records 16-byte aligned, the u32 arrays 4-byte.  The schedule is checked and uploaded with the call.  Asynchronous
 * on `stream`.  HM_ERR_BAD_ARG, with nothing launched: NULL arguments, n_proofs 0 or above 2^24, slots 0 or above 2^16, points >
 * slots, preamble_stride, record_elems or n_schedule_pairs 0 or above 2^16, a schedule whose absorbed slots do not sum to `slots` or
 * whose squeezes exceed record_elems, a buffer that is not aligned. */
int hm_blake2b512_dev(const void* d_msgs, size_t stride, const uint32_t* d_lens, size_t n, const uint8_t* personal16, void* d_out,
                      void* stream);
int hm_verify_transcript_dev(const void* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots, uint32_t points,
                             const void* d_y_bytes, const void* d_preamble, const uint32_t* d_preamble_counts, uint32_t preamble_stride,
                             const uint32_t* schedule, size_t n_schedule_pairs, uint32_t* d_bad_in_out, void* d_records,
                             uint32_t record_elems, void* stream);
/* The same three steps for proofs in the EVM encoding (snark-verifier's EvmTranscript, as recalled: csrc/keccak.inc and transcript.py
 * state the rules): a point stands uncompressed, x then y, 32 big-endian canonical bytes each, a scalar as 32 big-endian bytes, and
 * the transcript is Keccak-256 over the proof's own bytes.
 *
 * Keccak-256 (Keccak-f[1600], rate 136, padding byte 0x01 -- Ethereum's, not SHA-3's 0x06 --, 32-byte digest), one lane per message:
 * message i is the d_lens[i] bytes at d_msgs + i * stride (DEVICE memory, any alignment; d_lens: n u32, DEVICE memory); d_out: n x 32
 * digest bytes (DEVICE memory, 4-byte aligned).  A message whose length is above `stride` gets 32 zero bytes and nothing of it is
 * read.  Asynchronous on `stream`.  HM_ERR_BAD_ARG, with nothing launched: NULL arguments, n 0 or above 2^24, stride 0 or above
 * 2^32 - 1, d_lens or d_out not 4-byte aligned.
 *
 * read: as hm_verify_read_proofs_dev, one lane per (proof, 32-byte slot), on a table of its own kind (DEVICE memory, one u32 per
 * slot): bit 31 set on the x slot of a point, whose y is the next slot -- bits 0 .. 28 the point's index among the proof's own
 * points, or bit 30 for the tail --; bit 29 set on a y slot, which the lane of its x slot reads; neither set on a scalar, bits 0 ..
 * 28 its index.  A point is byte-reversed, both coordinates checked below p and the point on y^2 = x^3 + 3 (no square root), and
 * written as 8 u64 affine Montgomery words to row b * own_points + index of d_points_xy, or to row b of d_tail_xy; a scalar is
 * byte-reversed, checked below r and written as 4 Montgomery words to row b * scalars + index of d_scalars: bit for bit what
 * hm_verify_read_proofs_dev leaves for the same points and scalars.  There is no d_y_bytes.  A slot that cannot be read -- a
 * coordinate >= p, a point off the curve (the 64 zero bytes are one), a scalar >= r -- sets d_bad[b] and leaves zeros; a table entry
 * outside its array (a point index >= own_points without bit 30, a scalar index >= scalars, an x slot that is the proof's last)
 * sets d_bad[b], and nothing is read or written for it.  Asynchronous on `stream`.  HM_ERR_BAD_ARG, with nothing launched: NULL
 * arguments, n_proofs 0 or above 2^24, slots 0 or above 2^16, 2 own_points + scalars > slots, a buffer that is not aligned (d_proofs,
 * d_points_xy, d_tail_xy, d_scalars 16-byte; the u32 arrays 4-byte).
 *
 * transcript: one lane per proof.  Proof b absorbs d_preamble_counts[b] words from row b of d_preamble (n_proofs x preamble_stride x
 * 32 BIG-endian bytes: the digest of the verifying key, then the instance values), then walks `schedule` (HOST memory, pairs of u32:
 * absorb a slots, then squeeze s challenges; checked as hm_verify_transcript_dev checks its own) over its slots in order; a slot is
 * absorbed as the 32 bytes that stand in the proof.  A squeeze appends one byte 0x01 if and only if exactly 32 bytes were absorbed
 * since the last squeeze (the previous digest counts), pads, permutes, and restarts the sponge with the 32 digest bytes as its first
 * bytes; the digest, a big-endian integer, is reduced mod r.  Challenge j goes to element j of row b of d_records (n_proofs x
 * record_elems x 4 Montgomery words); the elements behind the schedule's challenges are left alone.  A proof whose d_bad_in_out[b] is
 * set on entry is not hashed and gets zero challenges; a preamble count above preamble_stride sets d_bad_in_out[b] with zero
 * challenges, and nothing is read outside the arrays.  The call needs nothing hm_verify_read_proofs_evm_dev writes but the flags, so
 * it may be queued before it.  All DEVICE memory but the schedule; d_proofs, d_preamble, d_records 16-byte aligned, the u32 arrays
 * 4-byte.  Asynchronous on `stream`.  HM_ERR_BAD_ARG, with nothing launched: NULL arguments, n_proofs 0 or above 2^24, slots,
 * preamble_stride, record_elems or n_schedule_pairs 0 or above 2^16, a schedule whose absorbed slots do not sum to `slots` or whose
 * squeezes exceed record_elems, a buffer that is not aligned. */
int hm_keccak256_dev(const void* d_msgs, size_t stride, const uint32_t* d_lens, size_t n, void* d_out, void* stream);
int hm_verify_read_proofs_evm_dev(const void* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots, uint32_t own_points,
                                  uint32_t scalars, void* d_points_xy, void* d_tail_xy, void* d_scalars, uint32_t* d_bad, void* stream);
int hm_verify_transcript_evm_dev(const void* d_proofs, size_t n_proofs, uint32_t slots, const void* d_preamble,
                                 const uint32_t* d_preamble_counts, uint32_t preamble_stride, const uint32_t* schedule,
                                 size_t n_schedule_pairs, uint32_t* d_bad_in_out, void* d_records, uint32_t record_elems, void* stream);

/* ---- pairing product checks: for every check c, is the product of e(P_i, Q_i) over its pairs 1? -------------------------------------
 *
 * The optimal ate pairing on BN256, one lane per pair for the Miller loops and one lane per check for the product and the final
 * exponentiation.  d_g1_xy: n_pairs x 8 u64, affine Montgomery words, (0, 0) = the identity.  d_g2_xy: n_pairs x 16 u64, the
 * Montgomery words of x.c0, x.c1, y.c0, y.c1 over Fq2 = Fq[u] / (u^2 + 1) on the twist y^2 = x^3 + 3 / (9 + u); sixteen zero words =
 * the identity.  d_offsets: n_checks + 1 entries; check c owns the pairs [d_offsets[c], d_offsets[c + 1]).
 * d_status[c]: 1 the product is 1 (an empty check, and one of identities only, is the product 1); 0 it is not; 2 the check holds a
 * malformed pair -- a coordinate word >= p, a point off its curve (no subgroup check on G2) -- or its offsets decrease or pass
 * n_pairs; such a pair is never multiplied in and nothing faults.  A pair with an identity on either side contributes 1.
 * d_gt: NULL, or n_checks x 48 u64: the value after the final exponentiation, the canonical Montgomery words of the 12 Fq of
 * ((a0, a1, a2), (b0, b1, b2)) in Fq12 = Fq6[w] / (w^2 - v), Fq6 = Fq2[v] / (v^3 - 9 - u); zeros with status 2.
 * d_work: hm_pairing_work_bytes(n_pairs, n_checks) bytes of DEVICE memory, 16-byte aligned, contents arbitrary: three Fq12 and a flag
 * word per pair, eleven Fq12 per check (the Miller values alone, n_pairs x 48 u64, do not suffice: an Fq12 never stands in registers).
 * All DEVICE memory; d_g1_xy, d_g2_xy, d_gt 16-byte aligned, d_offsets and d_status 4-byte.  Asynchronous on `stream`: two launches,
 * nothing read back.  HM_ERR_BAD_ARG, with nothing launched: NULL arguments (d_gt excepted), n_checks 0 or above 2^20, n_pairs above
 * 2^24, work_bytes below hm_pairing_work_bytes, a buffer that is not aligned.  hm_pairing_work_bytes is 0 outside those ranges. */
int hm_pairing_check_bn256_dev(const void* d_g1_xy, const void* d_g2_xy, size_t n_pairs, const uint32_t* d_offsets, size_t n_checks,
                               void* d_gt, uint32_t* d_status, void* d_work, size_t work_bytes, void* stream);
size_t hm_pairing_work_bytes(size_t n_pairs, size_t n_checks);

/* ---- introspection --------------------------------------------------------------------------- */

typedef struct hm_msm_stats {
  double digits_ms, sort_ms, accumulate_ms, reduce_ms, total_ms; /* hipEvent times of the last MSM */
  double accumulate_kernel_ms;                                   /* the bucket-accumulation launch alone */
  uint64_t pairs, tasks;                                         /* non-zero digits, accumulation tasks */
  uint32_t window_bits, windows;
} hm_msm_stats;
int hm_get_msm_stats(hm_msm_stats* out);

/* Per-call counters of the current device since start / hm_reset_stats: what a build of the Rust shim
 *  reads after create_proof to get the MEASURED call trace -- how many best_multiexp /
 * best_fft calls of which size, and where their time went. */
typedef struct hm_stats {
  uint64_t msm_calls, msm_points;         /* best_multiexp-equivalent calls (every form) and the points they covered */
  uint64_t ntt_calls, ntt_elements;       /* best_fft-equivalent transforms (a batched call of b arrays counts b) */
  uint64_t msm_calls_by_log2[32];         /* histogram over floor(log2 n) */
  uint64_t ntt_calls_by_log2[32];         /* histogram over log_n */
  double msm_h2d_us, msm_device_us, msm_host_us;  /* host-pointer uploads; SUM of the hipEvent spans of the launch chains (a grouped
                                                     chain counts once; chains in flight overlap: not a wall time); host fold */
  double ntt_h2d_us, ntt_device_us, ntt_d2h_us;   /* host-pointer form only (device-pointer calls are not waited for) */
  uint64_t h2d_bytes, d2h_bytes;          /* bytes the host-pointer forms moved over PCIe */
  /* the entry points beyond the two functions, by HM_STAT_* kind: calls (queries / lookups where a call carries several)
   * and the field elements they covered */
  uint64_t vector_calls[8], vector_elements[8];
  /* HBM the library holds between calls for the coset transforms' power tables (2^log_n x 32 B per (shift, log_n, form)): a
   * state, not a counter -- hm_reset_stats leaves it.  LRU, at most 48 tables and 2 GiB; given back on an allocation failure. */
  uint64_t coset_table_bytes, coset_tables;
  /* ... and for the twiddle tables of the transforms, one set per (omega, log_n): stage tables, and up to 2^21 a direct inter-pass
   * table of 2^log_n x 36 B (75 MB at 2^21).  LRU, at most 64 sets and 1 GiB. */
  uint64_t ntt_table_bytes, ntt_tables;
  /* The host-pointer forms' copies (csrc/xfer.hip), counted on this device since the library was loaded (hm_reset_stats leaves
   * them): copies handed to hipMemcpy on the caller's pointers (registered ranges, anything below 256 KiB, policy "direct"), copies
   * moved through the library's pinned staging lanes, and the ranges registered now (hm_host_register; process-wide). */
  uint64_t host_copies_direct, host_copies_staged, host_ranges_registered;
} hm_stats;
#define HM_STAT_EVAL_POLYNOMIAL 0
#define HM_STAT_GRAPH_EVALUATE 1
#define HM_STAT_KATE_DIVISION 2
#define HM_STAT_GRAND_PRODUCT 3
#define HM_STAT_BATCH_INVERT 4
#define HM_STAT_LINEAR_COMBINATION 5
#define HM_STAT_LOOKUP_PERMUTE 6
int hm_get_stats(hm_stats* out);
int hm_reset_stats(void);

#ifdef __cplusplus
}
#endif
#endif /* HALO2_MI355X_H */
