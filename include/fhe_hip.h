/*
 * fhe_hip.h -- C ABI of libfhe_hip.so: BFV ciphertext arithmetic on MI355X (gfx950).
 *
 * This is the drop-in boundary for the ONE hot path of wfus/Fully-Homomorphic-Image-Processing:
 * the arithmetic that homo/server_jpeg.cpp, server_resize.cpp and server_decode.cpp reach through
 * Microsoft SEAL v2.3's C++ class API (seal::Evaluator et al.).  The reference has no FFI of its
 * own; its seam is `#include "seal/seal.h"` (homo/fhe_image.h:13).  The SEAL-shaped C++ facade in
 * fully-homomorphic-image-processing_amd/seal/seal.h forwards every Evaluator call to the entry
 * points below, so homo/fhe_image.h, fhe_resize.h and fhe_decode.h compile unchanged against it.
 * INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types.  `stream` is a hipStream_t passed as void*
 *    (NULL = the default stream).  Device pointers are ordinary HIP device addresses (hipMalloc,
 *    torch.empty(device="cuda").data_ptr(), ...).  Calls are asynchronous on `stream`.
 *  - every function returns FHE_OK (0) or a negative error code; fhe_last_error() gives the text
 *    (thread-local).  Nothing throws.  There is NO CPU fallback: without a HIP device every
 *    compute entry point fails with FHE_ERR_HIP.
 *  - ciphertext layout (SEAL-logical): u64 [ciphertext][poly j][prime i][coeff c], every residue
 *    fully reduced to [0, q_i).  "n_polys" counts RNS polynomials, i.e. size * number of cts.
 *  - threading: a context is immutable for its users after fhe_ctx_create and may be shared by any number of
 *    host threads issuing calls on their own streams.  Two pieces of state are created later, both behind
 *    their own synchronisation and never freed or moved while the context lives: the ct x ct tables
 *    (auxiliary base, its twiddles, base-conversion constants), built under std::call_once by the FIRST
 *    entry point that multiplies ciphertexts (fhe_multiply*, fhe_square, fhe_relinearize,
 *    fhe_circuits_create, fhe_arith_path) -- threads racing that first call are safe, all see the same
 *    tables or the same error --, and the rgb_to_ycc constant cache (mutex-guarded).  Two restrictions:
 *    (1) the pipelined DCT mode (FHE_DCT_PIPELINE=1) uses one second stream owned by the context, so at most
 *    one fhe_dct8x8_quant call per context may be in flight in that mode; (2) fhe_ctx_destroy must not
 *    race with any other call on the same context.  Plans and scratch buffers belong to their caller.
 *  - devices: a context belongs to the device given to fhe_ctx_create; launches, fhe_dev_alloc and
 *    fhe_stream_create act on the CALLING THREAD's current HIP device.  fhe_ctx_create makes its device
 *    current for the creating thread; a host that drives several GPUs from one process uses one thread per
 *    device (or calls fhe_ctx_bind_thread before switching): seal/multi_gpu_dct.cpp is the worked example.
 *  - experiment switches (FHE_DCT_*, FHE_NTT_*, FHE_BEHZ_* environment variables; csrc/internal.h lists
 *    them) are read ONCE, by fhe_ctx_create, and are fixed for the life of that context: no launch path
 *    reads the environment.  The defaults are the measured-best kernels; every alternative gives the same
 *    bits (the parity tests create a second context with the variable set).  Creating a context costs a few
 *    milliseconds and a few MB of device tables (twiddles of the coefficient base; one stream and four
 *    events more in contexts created with FHE_DCT_PIPELINE=1); the ct x ct tables (twiddles for the k+1 auxiliary primes, base-conversion constants) are added
 *    by the first call that multiplies ciphertexts, so a DCT-only server neither pays for them nor can fail on
 *    the auxiliary-prime search (FHE_BEHZ_EAGER=1 builds them in fhe_ctx_create as before round 4).
 *  - "NTT form" buffers use a library-internal slot order; they are only meaningful to this
 *    library (produced by fhe_plain_prepare / fhe_ntt_forward, consumed by the matching calls).
 */
#ifndef FHE_HIP_H
#define FHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHE_OK 0
#define FHE_ERR_PARAM (-1)  /* invalid argument / unsupported parameter set   */
#define FHE_ERR_HIP (-2)    /* HIP runtime error (no device, launch failure)  */
#define FHE_ERR_NOMEM (-3)

#define FHE_MAX_K 8
#define FHE_MAX_POLYS 64      /* polynomials per ciphertext (the deepest reference circuit reaches 22, homo/fhe_decode.h:239) */

typedef struct fhe_ctx fhe_ctx;
typedef struct fhe_dct_plan fhe_dct_plan;
typedef void *fhe_stream;

const char *fhe_last_error(void);
/* ABI version of this header; bumped on any signature change and whenever entry points are added or a contract changes.
 *   1: rounds 1-3.
 *   2: + fhe_gather, fhe_host_alloc / fhe_host_free, fhe_stream_create / destroy, fhe_ctx_bind_thread / fhe_ctx_device,
 *      fhe_count_unreduced, fhe_add_sizes, the *_range / *_rows circuit shards, fhe_relinearize_to, the relinearised mode of the circuits
 *      (fhe_circuits_create_relin, fhe_circuits_out_size); fhe_ctx_create no longer builds or validates the ct x ct tables
 *      (auxiliary-prime failures surface at the first multiply or at fhe_circuits_create), fhe_arith_path builds them as
 *      a side effect, and the context's second stream exists only with FHE_DCT_PIPELINE=1.
 *   3: + fhe_encrypt_batch / fhe_encrypt_scratch_bytes / fhe_encrypt_draws / fhe_noise_cdt, fhe_frac_encode_batch,
 *      fhe_decrypt_batch / fhe_decrypt_scratch_bytes / fhe_ctx_modulus_bits.
 *   4: + fhe_relinearize_poly / fhe_relinearize_n (key switches for s^3 ..: a size-4 Cubic result goes to size 2 in one
 *      evaluator.relinearize, as SEAL's does), fhe_circuits_create_relin_at (include/fhe_circuits.h: where the relinearised mode
 *      relinearises); fhe_relinearize_to rejects partially overlapping input / output ranges.  Version 4 also carries
 *      fhe_idct_plan_create / destroy, fhe_idct8x8_scratch_bytes, fhe_idct8x8_dequant and fhe_ycc_to_rgb_blocks, added later:
 *      new entry points only, no existing signature or contract changed.  The same holds for the fhe_filter_* entry points (2-D convolution)
 *      and for fhe_weight_table_*, fhe_remap* and fhe_resample_axis_plan (resampling with public weights), and for fhe_batch_encode /
 *      fhe_batch_decode, fhe_galois_element and fhe_apply_galois (batched slots and Galois rotations), and for fhe_block8x8_plan_create /
 *      destroy, fhe_block8x8_scalar, fhe_channel_mix and fhe_dct8_matrix (integer linear maps across slot-packed ciphertexts), and for
 *      fhe_plane_map_plan_create / destroy / info and fhe_plane_map (sparse integer maps across position-packed ciphertexts), and for
 *      fhe_ctx_create_level and fhe_mod_switch (modulus switching: dropping RNS primes from ciphertexts), and for fhe_ksk_sp_words,
 *      fhe_key_switch_sp_scratch_bytes, fhe_relinearize_sp_poly and fhe_apply_galois_sp (key switching with a special prime), and for
 *      fhe_rotsum_plan_create / destroy, fhe_rotsum_scratch_bytes, fhe_rotate_sum_sp and fhe_rotate_each_sp (hoisted special-prime
 *      rotations of one ciphertext and their fused weighted sum), and for fhe_rotdiag_plan_create / destroy, fhe_rotdiag_scratch_bytes and
 *      fhe_rotate_diag_sum_sp (diagonal linear maps on encrypted slots: per-slot plaintext weights inside the fused sum), and for
 *      fhe_rotbsgs_plan_create / destroy, fhe_rotbsgs_scratch_bytes and fhe_rotate_bsgs_sp (baby-step / giant-step linear maps on encrypted
 *      slots: G1 + G2 keys for G1 G2 diagonals).
 * A host compiled against this header compares fhe_abi_version() with FHE_ABI_VERSION before anything else (the Python
 * binding and seal/seal.h do). */
#define FHE_ABI_VERSION 4
uint32_t fhe_abi_version(void);

/* ---- context: replaces seal::EncryptionParameters + seal::SEALContext -------------------------
 * (homo/server_jpeg.cpp:74-80: set_poly_modulus("1x^n + 1"), set_coeff_modulus(coeff_modulus_128(n)),
 *  set_plain_modulus(t)).  q_i must be distinct primes < 2^61 with q_i = 1 (mod 2n); n a power of
 * two in [1024, 16384].  Tables (twiddles, Shoup companions, BEHZ base-conversion constants) are
 * built on the host and uploaded to `device`. */
int fhe_ctx_create(uint32_t n, const uint64_t *q, uint32_t k, uint64_t t, int device, fhe_ctx **out);
int fhe_ctx_destroy(fhe_ctx *ctx);
/* The context a fhe_mod_switch result lives in: on the parent's device, with the parent's n and t, its first k_out primes (1 <= k_out < k) and
 * the experiment switches the parent was created with (the environment is not read again).  A context of its own: the caller destroys it,
 * before or after the parent.  A secret key [k][n] of the parent restricted to its first k_out rows is the same key there. */
int fhe_ctx_create_level(const fhe_ctx *parent, uint32_t k_out, fhe_ctx **out);
/* 1 once the lazily built ct x ct tables exist (diagnostic: a context that only ran linear circuits reports 0) */
int fhe_ctx_has_ctct_tables(const fhe_ctx *ctx);
/* the device the context was created on; fhe_ctx_bind_thread makes it the calling thread's current device (hipSetDevice) */
int fhe_ctx_device(const fhe_ctx *ctx);
int fhe_ctx_bind_thread(const fhe_ctx *ctx);
/* a non-blocking stream on the calling thread's current device, for hosts without HIP headers (pass it as `stream`) */
int fhe_stream_create(fhe_stream *out);
int fhe_stream_destroy(fhe_stream stream);
uint32_t fhe_ctx_n(const fhe_ctx *ctx);
uint32_t fhe_ctx_k(const fhe_ctx *ctx);
uint64_t fhe_ctx_t(const fhe_ctx *ctx);
uint64_t fhe_ctx_q(const fhe_ctx *ctx, uint32_t i);
/* SEAL 2.3 `coeff_modulus_128(n)` replacement (homo/server_jpeg.cpp:78).  preset 0 = the
 * 3x36/37-bit set BASELINE.json names for n=4096 (and the matching sets for other n),
 * preset 1 = SEAL 2.3.1 defaults.  Returns the number of primes written (<= FHE_MAX_K) or <0. */
int fhe_default_coeff_modulus(uint32_t n, int preset, uint64_t *q_out);

/* ---- device memory helpers for hosts without their own allocator (the C++ facade) ------------ */
int fhe_dev_alloc(size_t bytes, void **dptr);
int fhe_dev_free(void *dptr);
int fhe_upload(void *dst_dev, const void *src_host, size_t bytes, fhe_stream stream);
int fhe_download(void *dst_host, const void *src_dev, size_t bytes, fhe_stream stream);
int fhe_copy(void *dst_dev, const void *src_dev, size_t bytes, fhe_stream stream);
int fhe_stream_sync(fhe_stream stream);
/* page-locked host memory for staging buffers of hosts without their own allocator (the facade's Ciphertext::load / save go
 * through one per thread: a transfer from or to pageable memory is staged a second time inside the runtime) */
int fhe_host_alloc(size_t bytes, void **hptr);
int fhe_host_free(void *hptr);
/* `count` scattered device buffers (addresses in HOST memory, consumed before the call returns) of words_each u64 ->
 * dst[i * dst_stride_words ...], one launch per 256 sources, no staging copy.  The SEAL facade's lazy mode uses it to
 * run the reference's one-ciphertext-at-a-time Evaluator calls (homo/fhe_image.h:206-284) as batched launches.  16-byte
 * units: even word counts, 16-byte aligned buffers. */
int fhe_gather(const uint64_t *const *src_host, uint64_t count, uint64_t words_each, uint64_t *dst,
               uint64_t dst_stride_words, fhe_stream stream);

/* ---- seal::FractionalEncoder(t, poly_modulus, int_coeffs, frac_coeffs, base=2) ------------------
 * (ctor homo/server_jpeg.cpp:100; encode() call sites homo/fhe_image.h:221-236,259,301,317-319).
 * Host-side, no device work.  plain_out must hold n coefficients; returns the significant
 * coefficient count (0 for the zero plaintext) or <0. */
int fhe_frac_encode(uint32_t n, uint64_t t, double value, int int_coeffs, int frac_coeffs,
                    uint64_t *plain_out);
double fhe_frac_decode(uint32_t n, uint64_t t, const uint64_t *plain, int int_coeffs, int frac_coeffs);

/* ---- seal::Evaluator::add / sub / negate (homo/fhe_image.h:207-220, fhe_resize.h:151-169,
 * fhe_decode.h:219).  Element-wise over n_polys RNS polynomials; out may alias a or b.
 * Unequal ciphertext sizes are handled by the caller (facade) by running the common prefix
 * through add/sub and the tail through copy/negate, as SEAL does. */
int fhe_add(const fhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n_polys,
            fhe_stream stream);
int fhe_sub(const fhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n_polys,
            fhe_stream stream);
int fhe_negate(const fhe_ctx *ctx, const uint64_t *a, uint64_t *out, uint64_t n_polys, fhe_stream stream);
/* The same add / sub for `count` pairs of ciphertexts of UNEQUAL sizes, batched (a: [count][size_a][k][n], b: [count][size_b][k][n],
 * out: [count][max(size_a, size_b)][k][n]): the destination grows and the polynomials the shorter operand lacks count as zero
 * (sub: the tail of b is negated), as seal::Evaluator does at homo/fhe_resize.h:181-184 and homo/fhe_decode.h:114-118,237 where a
 * size-3 product meets a size-2 or a size-5 ciphertext.  out may alias the longer operand.  subtract: 0 = a + b, 1 = a - b. */
int fhe_add_sizes(const fhe_ctx *ctx, const uint64_t *a, uint32_t size_a, const uint64_t *b, uint32_t size_b, uint64_t *out,
                  uint64_t count, int subtract, fhe_stream stream);

/* ---- plaintext operands ---------------------------------------------------------------------------
 * fhe_plain_prepare: centred lift of a seal::Plaintext (coefficients in [0,t), host memory) to the
 * q-base followed by a forward NTT; writes 2*k*n u64 to d_plain_ntt (value + Shoup companion per
 * slot).  Cache the result: the reference re-encodes and re-transforms the same 13 constants on
 * every call (homo/fhe_image.h:221-236). */
size_t fhe_plain_ntt_words(const fhe_ctx *ctx);
int fhe_plain_prepare(const fhe_ctx *ctx, const uint64_t *plain_host, uint32_t plain_len,
                      uint64_t *d_plain_ntt, fhe_stream stream);
/* product of two prepared plaintexts as ring elements (used to fold encode(0.125)*encode(1/q)) */
int fhe_plain_ntt_mul(const fhe_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out,
                      fhe_stream stream);

/* seal::Evaluator::multiply_plain (homo/fhe_image.h:221 etc.): every polynomial of the n_polys
 * inputs is multiplied in R_q by the prepared plaintext (fused NTT -> dyadic -> inverse NTT).
 * n_polys must be a multiple of k (whole RNS polynomials).  out may alias in. */
int fhe_multiply_plain(const fhe_ctx *ctx, const uint64_t *in, uint64_t *out, uint64_t n_polys,
                       const uint64_t *d_plain_ntt, fhe_stream stream);
/* multiply_plain for a plaintext with at most FHE_SPARSE_MAX_TERMS non-zero coefficients (host
 * memory, coefficients in [0,t)): the ring product is formed directly as a sum of signed rotations
 * in coefficient form -- no transform.  The integer and power-of-two constants of Cubic
 * (encode(3) = x+1, encode(5) = x^2+1, encode(0.5) = -x^(n-1); homo/fhe_resize.h:150-163,186) are of
 * this kind.  Same result as fhe_multiply_plain (exact ring arithmetic, canonical residues).
 * out may alias in.  n <= 8192.  Returns FHE_ERR_PARAM if the plaintext has more terms or is zero. */
#define FHE_SPARSE_MAX_TERMS 8
int fhe_multiply_plain_sparse(const fhe_ctx *ctx, const uint64_t *in, uint64_t *out, uint64_t n_polys,
                              const uint64_t *plain_host, uint32_t plain_len, fhe_stream stream);

/* Cubic (homo/fhe_resize.h:143-189) outside its four ciphertext products, for FractionalEncoder base 2
 * where encode(3) = x+1, encode(2) = x, encode(5) = x^2+1, encode(4) = x^2, encode(0.5) = -x^(n-1):
 *   fhe_cubic_coeffs:  a = 3B - A - 3C + D,  b = 2A - 5B + 4C - D,  c = C - A      (:150-172; one pass
 *                      over A..D instead of six multiply_plain and eight add/sub calls)
 *   fhe_cubic_combine: out = 0.5 (a + b + c) + B                                   (:181-188)
 * exactly as the Evaluator calls compose (same ring elements, canonical residues).  Operands are
 * batches of `count` ciphertexts; A..D, a, b, c have `size` polynomials each; in combine a, b, c have
 * `size_abc` polynomials, B has `size_b` <= size_abc, out has size_abc.  Outputs must not alias inputs. */
int fhe_cubic_coeffs(const fhe_ctx *ctx, const uint64_t *A, const uint64_t *B, const uint64_t *C, const uint64_t *D,
                     uint64_t *a, uint64_t *b, uint64_t *c, uint32_t size, uint64_t count, fhe_stream stream);
int fhe_cubic_combine(const fhe_ctx *ctx, const uint64_t *a, const uint64_t *b, const uint64_t *c, uint32_t size_abc,
                      const uint64_t *B, uint32_t size_b, uint64_t *out, uint64_t count, fhe_stream stream);

/* seal::Evaluator::add_plain / sub_plain (homo/fhe_image.h:317 sub_plain(128.0); fhe_resize.h:196;
 * fhe_decode.h:57,113,218,220,229): c_0 += sign * Delta * m' for `count` ciphertexts whose first
 * polynomial starts every ct_stride_words u64. sign = +1 / -1. */
int fhe_add_plain(const fhe_ctx *ctx, uint64_t *ct, uint64_t ct_stride_words, uint64_t count,
                  const uint64_t *plain_host, uint32_t plain_len, int sign, fhe_stream stream);

/* ---- negacyclic NTT over the q-base (north_star primitive; SEAL-internal in the reference) -----
 * in: [n_polys][k][n] coefficient form; out: NTT form (internal slot order), values in [0,q_i). */
int fhe_ntt_forward(const fhe_ctx *ctx, const uint64_t *in, uint64_t *out, uint64_t n_polys,
                    fhe_stream stream);
int fhe_ntt_inverse(const fhe_ctx *ctx, const uint64_t *in, uint64_t *out, uint64_t n_polys,
                    fhe_stream stream);
/* coefficient-wise (dyadic) product of two NTT-form operands with Barrett reduction */
int fhe_dyadic_multiply(const fhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out,
                        uint64_t n_polys, fhe_stream stream);

/* ---- seal::Evaluator::multiply / square (homo/fhe_resize.h:174-179,197-198; fhe_decode.h:67-97,
 * 235,239): full-RNS BEHZ product of `count` pairs of ciphertexts of sizes size_a, size_b
 * (each operand contiguous, [count][size][k][n]); out has size_a+size_b-1 polys per pair.
 * scratch: device memory of at least fhe_multiply_scratch_bytes(). */
size_t fhe_multiply_scratch_bytes(const fhe_ctx *ctx, uint32_t size_a, uint32_t size_b, uint64_t count);
int fhe_multiply(const fhe_ctx *ctx, const uint64_t *a, uint32_t size_a, const uint64_t *b,
                 uint32_t size_b, uint64_t *out, uint64_t count, void *scratch, size_t scratch_bytes,
                 fhe_stream stream);
int fhe_square(const fhe_ctx *ctx, const uint64_t *a, uint32_t size_a, uint64_t *out, uint64_t count,
               void *scratch, size_t scratch_bytes, fhe_stream stream);
/* An operand of fhe_multiply extended to the auxiliary base and transformed ONCE, for circuits that
 * multiply several ciphertexts by the same one (Cubic: t and t^2 enter every row of a pixel,
 * homo/fhe_resize.h:176-179,296-303).  fhe_multiply(a, b) == fhe_multiply_prepared(prepare(a), prepare(b))
 * bit for bit.  A prepared operand holds fhe_multiply_operand_words() u64 words in device memory and is
 * opaque.  Pass NULL for a_prepared (b_prepared) together with the plain ciphertext a (b) to prepare that
 * side inside the call. */
size_t fhe_multiply_operand_words(const fhe_ctx *ctx, uint32_t size, uint64_t count);
int fhe_multiply_prepare(const fhe_ctx *ctx, const uint64_t *a, uint32_t size, uint64_t count, uint64_t *prepared,
                         fhe_stream stream);
int fhe_multiply_prepared(const fhe_ctx *ctx, const uint64_t *a, const uint64_t *a_prepared, uint32_t size_a,
                          const uint64_t *b, const uint64_t *b_prepared, uint32_t size_b, uint64_t *out, uint64_t count,
                          void *scratch, size_t scratch_bytes, fhe_stream stream);
/* The same with a prepared operand batch SHARED between the pairs: b_prepared holds b_count entries and pair c
 * multiplies entry (b_first + c / b_div) % b_count -- ResizeImage's offsets (homo/fhe_resize.h:351,382): frac(u) depends
 * on the output column only and frac(v) on the output row only, so a batch of whole pixel rows in row-major order
 * multiplies xfract[c % width] (b_div = 1, b_count = width) and yfract[first_row + c / width] (b_div = width).
 * Bit-identical to fhe_multiply_prepared on the gathered operand; no copy of the prepared words is made. */
int fhe_multiply_prepared_shared(const fhe_ctx *ctx, const uint64_t *a, const uint64_t *a_prepared, uint32_t size_a,
                                 const uint64_t *b_prepared, uint32_t size_b, uint64_t b_count, uint64_t b_div,
                                 uint64_t b_first, uint64_t *out, uint64_t count, void *scratch, size_t scratch_bytes,
                                 fhe_stream stream);

/* ---- seal::Evaluator::relinearize (north_star API surface; the reference never calls it, only
 * tests/parameters.cpp:112 touches evaluation keys).  Key-switch inner product for `count`
 * size-3 ciphertexts -> size 2, in place on the first two polys.  evk (device):
 * [k][n_digits][2][k][n] in NTT form (internal order) as produced by fhe_evk_to_ntt. */
uint32_t fhe_evk_digits(const fhe_ctx *ctx, uint32_t dbc);
int fhe_relinearize(const fhe_ctx *ctx, uint64_t *ct3, uint64_t ct_stride_words, uint64_t count,
                    const uint64_t *d_evk_ntt, uint32_t dbc, void *scratch, size_t scratch_bytes,
                    fhe_stream stream);
size_t fhe_relinearize_scratch_bytes(const fhe_ctx *ctx, uint32_t dbc, uint64_t count);
/* The same with the result written elsewhere: out2[c * out_stride_words ...] = the relinearised size-2 ciphertext of
 * ct3[c * ct_stride_words ...] (a batch of products becomes a compact [count][2][k][n] batch without a copy of its own;
 * the relinearised mode of the circuits, include/fhe_circuits.h, is built on it).  out2 == ct3 with equal strides is
 * fhe_relinearize.  Same scratch.  Aliasing rule: the output range [out2, out2 + (count-1) out_stride + 2kn) either IS the
 * input (same pointer, same stride) or does not overlap [ct3, ct3 + (count-1) stride + 3kn) at all; any other overlap
 * returns FHE_ERR_PARAM (a compacting in-place relinearisation would let one ciphertext's output land on another's input). */
int fhe_relinearize_to(const fhe_ctx *ctx, const uint64_t *ct3, uint64_t ct_stride_words, uint64_t *out2,
                       uint64_t out_stride_words, uint64_t count, const uint64_t *d_evk_ntt, uint32_t dbc, void *scratch,
                       size_t scratch_bytes, fhe_stream stream);

/* One key-switch step (what SEAL 2.3's relinearize repeats until size 2): polynomial `src_poly` >= 2 -- the LAST one of a
 * ciphertext of src_poly + 1 polynomials -- is decomposed into digits and folded into c0 / c1 with the keys for
 * s^src_poly (d_evk_ntt: [k][n_digits][2][k][n], same form as above, made from s^src_poly instead of s^2).  Only c0' and c1'
 * are written (out2, same aliasing rule as fhe_relinearize_to); in place (out2 == ct, equal strides) polynomials
 * 2 .. src_poly - 1 simply stay where they are, so the ciphertext has become one polynomial shorter.  src_poly == 2 is
 * fhe_relinearize_to.  Same scratch. */
int fhe_relinearize_poly(const fhe_ctx *ctx, const uint64_t *ct, uint64_t ct_stride_words, uint32_t src_poly, uint64_t *out2,
                         uint64_t out_stride_words, uint64_t count, const uint64_t *d_evk_ntt, uint32_t dbc, void *scratch,
                         size_t scratch_bytes, fhe_stream stream);
/* evaluator.relinearize(ct, evk) for ciphertexts of `size` >= 3 polynomials down to 2 (SEAL 2.3: size - 2 steps, the top
 * polynomial first): d_evk_ntt holds the keys for s^2, s^3, .. s^(size-1) one after the other (fhe_evk_words(ctx, dbc) words
 * each; KeyGenerator::generate_evaluation_keys(dbc, size - 2, keys)).  The steps above the last one run IN PLACE: ct's first two
 * polynomials are overwritten with partial sums when size > 3 (ct is scratch after the call).  out2 as in fhe_relinearize_to. */
size_t fhe_evk_words(const fhe_ctx *ctx, uint32_t dbc);
/* scratch for fhe_relinearize_n: the digits of all size - 2 source polynomials at once.  With at least this much the size - 2 key
 * switches run in as few PASSES as the lazy sums of the pseudo-Mersenne kernels allow (k * digits * powers <= 20 terms per pass: one
 * pass for a size-4 ciphertext at k = 4, dbc 30, and for a size-6 one at dbc 60; two passes of two powers for size 6 at dbc 30) --
 * every step's source polynomial is the caller's own, so the result is the ciphertext plus the sum of the steps' terms, the same bits
 * in any order -- with one inverse transform pair per pass instead of one per step; with only fhe_relinearize_scratch_bytes the steps
 * run one after the other. */
size_t fhe_relinearize_n_scratch_bytes(const fhe_ctx *ctx, uint32_t size, uint32_t dbc, uint64_t count);
int fhe_relinearize_n(const fhe_ctx *ctx, uint64_t *ct, uint32_t size, uint64_t ct_stride_words, uint64_t *out2,
                      uint64_t out_stride_words, uint64_t count, const uint64_t *d_evk_ntt, uint32_t dbc, void *scratch,
                      size_t scratch_bytes, fhe_stream stream);

/* ---- batched plaintext slots and Galois rotations: seal::PolyCRTBuilder, seal::GaloisKeys, seal::Evaluator::rotate_rows /
 * rotate_columns (SEAL 2.3; the reference never calls them: every pixel of its streams is one ciphertext).  New entry points only.
 *
 * Slots.  For a PRIME plain modulus t = 1 (mod 2n) the plaintext ring splits into n slots: with zeta the SMALLEST primitive 2n-th root
 * of unity modulo t, slot (r, j), r in {0, 1}, 0 <= j < n/2, of a plaintext m is m(zeta^e) mod t, e = 3^j mod 2n for row 0 and
 * e = 2n - 3^j mod 2n for row 1; the flat slot order is row 0, then row 1.  add / sub / multiply_plain / multiply / square act slot by slot.
 * fhe_batch_encode writes the `count` plaintexts (n coefficients below t each) whose slots are the given values, fhe_batch_decode
 * evaluates them: an inverse and a forward number-theoretic transform modulo t on the host, no device.  FHE_ERR_PARAM for a t that is
 * not prime or not 1 mod 2n (the presets' 2^14 is refused), a t of more than 60 bits, and a value >= t. */
int fhe_batch_encode(uint32_t n, uint64_t t, const uint64_t *slots, uint64_t count, uint64_t *plain);
int fhe_batch_decode(uint32_t n, uint64_t t, const uint64_t *plain, uint64_t count, uint64_t *slots);
/* Automorphism.  For odd g in (1, 2n), sigma_g maps x^i to x^(i g mod 2n) with x^n = -1: coefficient i of the input goes to position
 * e = i g mod 2n if e < n, otherwise to position e - n NEGATED modulo q_i (the negation of 0 is 0, not q_i).  On the slots above
 * sigma_g with g = 3^s mod 2n rotates both rows LEFT by s (slot (r, j) of the result is slot (r, j + s mod n/2) of the input) and
 * g = 2n - 1 swaps the rows.  fhe_galois_element (host only) gives g = 3^steps mod 2n -- the inverse power for negative steps; steps
 * count modulo n/2 --, times 2n - 1 if swap_rows != 0; steps == 0 without the swap gives 1, the identity, which fhe_apply_galois refuses. */
int fhe_galois_element(uint32_t n, int steps, int swap_rows, uint32_t *g);
/* apply_galois(ct, g, key_g) for `count` ciphertexts of size 2 (other sizes are refused by the hosts, as SEAL 2.3 does):
 *     out = relinearize-step([sigma_g(c0), 0, sigma_g(c1)])
 * i.e. the digits of sigma_g(c1)'s residues (dbc bits each, per source prime: exactly fhe_relinearize_poly's rule with src_poly = 2)
 * are multiplied with key_g and added to (sigma_g(c0), 0).  d_key_ntt: [k][digits][2][k][n] in NTT form, fhe_evk_words(ctx, dbc) words,
 * made like the evaluation key for s^2 but for the target sigma_g(s): entry (i, d) = (-(a s + e) + 2^(dbc d) sigma_g(s) on component i
 * only, a).  ct2 [c * ct_stride_words ...] -> out2[c * out_stride_words ...]; aliasing rule of fhe_relinearize_to: out2 IS the input
 * (same pointer, same stride) or does not overlap it.  Bit-identical to that composition on every context (csrc/galois.hip: the
 * kernels read their source polynomials through the automorphism; FHE_GALOIS_STAGED=1 at fhe_ctx_create materialises
 * [sigma(c0), 0, sigma(c1)] in scratch and runs fhe_relinearize_poly on it).  Everything is checked before anything is enqueued: g even,
 * g == 1, g >= 2n, strides below 2 k n, short scratch, a forbidden overlap of input, output and scratch: FHE_ERR_PARAM.  count == 0 is
 * a no-op. */
size_t fhe_apply_galois_scratch_bytes(const fhe_ctx *ctx, uint32_t dbc, uint64_t count);
int fhe_apply_galois(const fhe_ctx *ctx, const uint64_t *ct2, uint64_t ct_stride_words, uint64_t *out2, uint64_t out_stride_words,
                     uint64_t count, uint32_t galois_elt, const uint64_t *d_key_ntt, uint32_t dbc, void *scratch, size_t scratch_bytes,
                     fhe_stream stream);

/* ---- integer linear maps ACROSS slot-packed ciphertexts: the packed JPEG transform ------------------------------------------------
 * A client that packs by POSITION -- ciphertext p = 8 r + c of a group of 64 holds, in slot b, pixel (r, c) of 8x8 block b -- turns the block
 * DCT, the quantisation, their inverses and the colour conversion into linear maps across ciphertexts with integer SCALAR weights: no
 * rotation, no key.  New entry points only.
 *
 * Scalars.  A scalar is an int64_t w; it acts on a polynomial as multiply_plain with the one-coefficient plaintext [w mod t], i.e. as the
 * coefficient-wise product modulo each q_i with the centred lift of w mod t (fhe_multiply_plain_sparse's rule).  Every scalar must satisfy
 * |w| <= min((t - 1) / 2, 2^31 - 1), so that the lift of w is w itself; anything else is FHE_ERR_PARAM.  Zero entries of a matrix are skipped
 * terms.  The ring operations are exact and residues canonical, so any order of evaluation and any folding of constants modulo q_i gives the
 * same bits: "bit-identical" below is to the op-by-op composition of multiply_plain and add.
 *
 * fhe_block8x8_scalar: in, out [count][64][size][k][n], size >= 2 polynomials per ciphertext; ciphertext 8 x + y of a group is X[x][y].  For
 * every polynomial, prime and coefficient
 *     Y[u][v] = post[u][v] * sum_x sum_y L[u][x] * R[v][y] * pre[x][y] * X[x][y]        (mod q_i, canonical)
 * bit-identical to: pre per input, L down the columns, R along the rows, post per output.  L, R, pre, post: [64] row-major host arrays;
 * pre / post == NULL mean all ones.  fhe_block8x8_plan_create refuses (FHE_ERR_PARAM) a zero entry of pre or post, an all-zero row of L or R
 * (an output that would be the transparent zero), a scalar out of range and a null pointer; fhe_block8x8_scalar refuses size < 2,
 * size > FHE_MAX_POLYS, a null pointer, a plan of another context and an output that overlaps the input without being it -- all before
 * anything is enqueued.  out == in is allowed; count == 0 is a no-op.  No scratch: one kernel reads each input word once and writes each output
 * word once (csrc/packed.hip).  The plan
 * keeps 4 x 64 constants per prime on the device and belongs to its context. */
typedef struct fhe_block8x8_plan fhe_block8x8_plan;
int fhe_block8x8_plan_create(const fhe_ctx *ctx, const int64_t *L, const int64_t *R, const int64_t *pre, const int64_t *post, fhe_stream stream,
                             fhe_block8x8_plan **out);
int fhe_block8x8_plan_destroy(fhe_block8x8_plan *plan);
int fhe_block8x8_scalar(const fhe_ctx *ctx, const fhe_block8x8_plan *plan, const uint64_t *in, uint64_t *out, uint32_t size, uint64_t count,
                        fhe_stream stream);
/* out_i = sum_j M[i][j] * in_j for `count` ciphertexts of `size` polynomials in each of c input and m output planes, 1 <= c, m <= 8 (M: [m][c]
 * row-major host scalars): ciphertext e of input channel j starts at in + e * in_ct_stride_words + j * in_plane_stride_words, outputs likewise
 * (interleaved and planar layouts are both strides).  With bias != NULL, fhe_add_plain with the one-coefficient plaintext [bias_i mod t],
 * sign +1, follows on output plane i (the bias range is the scalar range; a zero bias adds nothing).  An all-zero row of M is refused.  In
 * place is allowed when the pointers and strides are identical and m == c; any other overlap of the input and output ranges, and strides that
 * let two ciphertexts of one operand overlap, are refused.  count == 0 is a no-op. */
int fhe_channel_mix(const fhe_ctx *ctx, const int64_t *M, const int64_t *bias, uint32_t c, uint32_t m, const uint64_t *in,
                    uint64_t in_ct_stride_words, uint64_t in_plane_stride_words, uint64_t *out, uint64_t out_ct_stride_words,
                    uint64_t out_plane_stride_words, uint32_t size, uint64_t count, fhe_stream stream);
/* Host only: D[u][x] = round-half-away-from-zero(2^bits * c_u / 2 * cos((2 x + 1) u pi / 16)), c_0 = 1 / sqrt(2), c_u = 1 otherwise -- the
 * orthonormal 8-point DCT-II in `bits` fractional bits, 1 <= bits <= 20, D: [64] row-major.  bits = 8: row 0 is eight times 91, row 1 is
 * 126, 106, 71, 25, -25, -71, -106, -126.  Row u is (-1)^u-symmetric.  The fixed-point transform built from it (circuits.packed_dct_plan) is a
 * transform of its own: its ciphertexts and decrypted values are NOT those of fhe_dct8x8_quant below, which follows the reference's
 * FractionalEncoder circuit. */
int fhe_dct8_matrix(int bits, int64_t *D);

/* ---- sparse integer maps across position-packed ciphertexts: packed resize, warps, tile filters -------------------------------------
 * A client that packs by POSITION -- ciphertext p of a frame of n_in ciphertexts holds, in slot b, pixel p of frame (or tile) b -- turns a
 * resize, a warp, a strided filter or a chroma subsampling into one sparse linear map across ciphertexts with integer scalar weights (the
 * scalar rule above): no transform, no rotation, no key.  New entry points only.
 *
 * fhe_plane_map: in [count][n_in][size][k][n], out [count][n_out][size][k][n].  For output plane o, visiting slots p = 0 .. T - 1 in order:
 * a slot of weight 0 is skipped (its tap is not looked at); otherwise the term is multiply_plain(in[taps[o][p]], [weights[o][p] mod t]); the
 * terms are combined with add.  The result has `size` polynomials, is fully reduced and is bit-identical to that composition (exact ring
 * operations: any order of evaluation gives the same bits).  A source may appear twice in one output: two terms.
 *
 * fhe_plane_map_plan_create refuses (FHE_ERR_PARAM): an output with no live term (the transparent zero), a live tap >= n_in, T outside
 * 1 .. FHE_PLANE_MAX_TAPS, n_in or n_out of 0 or above FHE_PLANE_MAX_PLANES, a window other than 0, 16, 32, 64, an order that is not a
 * permutation of 0 .. n_out - 1, a scalar out of range, a null pointer (order may be NULL: index order).  fhe_plane_map refuses size < 2,
 * size > FHE_MAX_POLYS, a null pointer, a plan of another context and an output range that overlaps the input range in any way (the plane
 * counts differ: there is no in-place form) -- all before anything is enqueued.  count == 0 is a no-op.  No scratch.
 *
 * Groups.  The plan cuts the outputs into groups; the kernel loads the distinct live sources of a group once (at most 64 words per thread,
 * in LDS) and forms the group's outputs from them (csrc/planemap.hip).  The cut is made in plan_create and is the same on every host: walk
 * the outputs in `order` (index order when NULL); an output joins the open group while the union of the group's live sources stays <=
 * window, otherwise the group is closed and the output opens the next one.  An output with more live sources than the window (at most 64:
 * T <= 64) still gets a group of its own -- the window is raised to 64 for that group.  window 0 = the library's default, 16
 * (FHE_PLANEMAP_WINDOW in the environment of fhe_ctx_create overrides it).  The bits do not depend on the cut.  fhe_plane_map_plan_info
 * reports the number of groups, source_reads = the sum over groups of their distinct sources (read amplification = source_reads / distinct
 * sources used) and the window of the cut; any of the three pointers may be NULL.  The plan keeps its tables on the device and belongs to
 * its context.
 * Which kernel runs.  A plan created with window 0 runs the direct kernel (one thread per output word, sources from global memory, the
 * groups unused): it measured faster than the windowed one in two of six cases.  A plan created with an explicit window, and every plan of
 * a context created with FHE_PLANEMAP_WINDOW=16|32|64, runs the windowed kernel; FHE_PLANEMAP_DIRECT=1 forces the direct one.  Same bits. */
#define FHE_PLANE_MAX_TAPS 64
#define FHE_PLANE_MAX_PLANES 65536
typedef struct fhe_plane_map_plan fhe_plane_map_plan;
int fhe_plane_map_plan_create(const fhe_ctx *ctx, uint32_t n_in, uint32_t n_out, uint32_t T, const uint32_t *taps, const int64_t *weights,
                              const uint32_t *order, uint32_t window, fhe_stream stream, fhe_plane_map_plan **out);
int fhe_plane_map_plan_destroy(fhe_plane_map_plan *plan);
int fhe_plane_map_plan_info(const fhe_plane_map_plan *plan, uint32_t *groups, uint64_t *source_reads, uint32_t *window);
int fhe_plane_map(const fhe_ctx *ctx, const fhe_plane_map_plan *plan, const uint64_t *in, uint64_t *out, uint32_t size, uint64_t count,
                  fhe_stream stream);

/* ---- modulus switching: drop the last primes of the coefficient modulus -----------------------------------------------------------
 * A result that has budget to spare does not need all k primes: switched to the first k_out it decrypts to the same plaintext under the
 * same secret key (restricted to those primes) in a context made by fhe_ctx_create_level, with k_out / k of the bytes.  New entry points only.
 *
 * One drop removes the last prime p = q_m of a base q_0 .. q_m, per coefficient: with c the canonical representative in [0, q) and
 * h = floor(p / 2),  c' = floor((c + h) / p) mod (q / p);  in residues, with r = (c_m + h) mod p, for i < m
 *     c'_i = (c_i + (h mod q_i) - (r mod q_i)) * p^-1 mod q_i        (fully reduced)
 * (SEAL 3.x divide_and_round_q_last).  fhe_mod_switch: in [n_polys][k][n] -> out [n_polys][k_out][n] is that drop applied k - k_out times,
 * last prime first, to every coefficient of every polynomial: the iteration is the definition, not one rounding by the product of the
 * dropped primes.  One kernel, no scratch, no allocation (csrc/modswitch.hip).
 * Noise: a ciphertext of `size` polynomials under a ternary secret with invariant noise budget B has, after the switch, at least
 *     -log2(2^-B + sum over the bases q' passed through of t S / q'),   S = 1 + n + .. + n^(size - 1)
 * bits (circuits.mod_switch_budget in the Python host).
 * Refused (FHE_ERR_PARAM) before anything is enqueued: k_out == 0 or k_out >= k, a null pointer, any overlap of the input and output ranges
 * (the strides differ: there is no in-place form).  n_polys == 0 is a no-op. */
int fhe_mod_switch(const fhe_ctx *ctx, uint32_t k_out, const uint64_t *in, uint64_t *out, uint64_t n_polys, fhe_stream stream);

/* ---- key switching with a special prime: relinearisation steps and Galois rotations without a digit decomposition ----------------------
 * The key switches above cut every source residue into digits of dbc bits: k * digits * k forward transforms, and a noise that grows with
 * 2^dbc.  Here the LAST prime of the context is the special prime p = q_(k-1); ciphertexts live on the first L = k - 1 primes
 * ([size][L][n], canonical residues: they belong to the context fhe_ctx_create_level(ctx, k - 1) makes and decrypt there under sk[:L]), keys
 * are made in ctx over all k primes, the key-switch product is formed modulo all k primes and then divided by p with rounding: L * k forward
 * transforms and 2 k inverse ones, and a noise of a few bits whatever the primes' size.  New entry points only (csrc/keyswitch_sp.hip).
 *
 * The key for a target polynomial T (s^j, or sigma_g(s), as residues over all k primes): [L][2][k][n] in NTT form (fhe_ntt_forward of ctx),
 * fhe_ksk_sp_words(ctx) = L * 2 * k * n words (0 when k < 2); entry i = (-(a_i s + e_i) + P_i T, a_i), a_i uniform, e_i noise, where "+ P_i T"
 * adds (p mod q_i) * T mod q_i on component i and nothing on any other component, the special prime's included
 * (P_i = p * (Q / q_i) * [(Q / q_i)^-1]_(q_i) reduced modulo each prime, Q = q_0 .. q_(L-1)).
 *
 * KS(d, K) of a source polynomial d [L][n] (coefficient form, canonical), for pp in {0, 1}:
 *   1. for every r < k:  acc_pp,r = sum_(i < L) [d_i]_(q_r) (*) K_i,pp,r  mod q_r, (*) the negacyclic product and [d_i]_(q_r) the integer
 *      d_i[c] in [0, q_i) reduced modulo q_r, coefficient by coefficient (not centred; d_i itself for r == i);
 *   2. u_pp = one drop of fhe_mod_switch, k -> k - 1 primes, applied to acc_pp (bit for bit).
 * fhe_relinearize_sp_poly (src_poly >= 2):  out = (c_0 + u_0, c_1 + u_1),  u = KS(c_src_poly, the key for s^src_poly); ct is
 *   [count] ciphertexts of at least src_poly + 1 polynomials.
 * fhe_apply_galois_sp (g odd in (1, 2n)):   out = (sigma_g(c_0) + u_0, u_1),  u = KS(sigma_g(c_1), the key for sigma_g(s)); sigma_g as above:
 *   the negation is modulo the SOURCE prime q_i, before the reduction to q_r, and the negation of 0 is 0.
 * Additions are modulo q_r and fully reduced.  ct at ct_stride_words, out2 [2][L][n] at out_stride_words; out2 either IS the input (same
 * pointer and stride: in place) or overlaps neither the input nor the scratch (the rule of fhe_relinearize_to).
 * Noise: one switch adds at most E = n B sum_(i < L) (q_i - 1) / p + (1 + n) / 2 to the numerator of the invariant noise (B the largest
 * noise sample): budget after >= -log2(2^-before + 2 t E / Q)  (circuits.special_key_switch_budget in the Python host).
 * Refused (FHE_ERR_PARAM) before anything is enqueued: k < 2, a null pointer, src_poly < 2, g even / 1 / >= 2n, a stride below the
 * ciphertext size, scratch_bytes < fhe_key_switch_sp_scratch_bytes(ctx, count), a forbidden overlap.  count == 0 is a no-op.  No device
 * allocation inside a call. */
size_t fhe_ksk_sp_words(const fhe_ctx *ctx);
size_t fhe_key_switch_sp_scratch_bytes(const fhe_ctx *ctx, uint64_t count);
int fhe_relinearize_sp_poly(const fhe_ctx *ctx, const uint64_t *ct, uint64_t ct_stride_words, uint32_t src_poly, uint64_t *out2,
                            uint64_t out_stride_words, uint64_t count, const uint64_t *d_key_ntt, void *scratch, size_t scratch_bytes,
                            fhe_stream stream);
int fhe_apply_galois_sp(const fhe_ctx *ctx, const uint64_t *ct2, uint64_t ct_stride_words, uint64_t *out2, uint64_t out_stride_words,
                        uint64_t count, uint32_t galois_elt, const uint64_t *d_key_ntt, void *scratch, size_t scratch_bytes, fhe_stream stream);

/* ---- hoisted special-prime rotations of ONE ciphertext and their fused weighted sum (csrc/rotsum.hip) ---------------------------------------
 * The setting is the one above: ctx has k >= 2 primes, the last one is the special prime, ciphertexts [2][L][n] live on the first L = k - 1,
 * keys are [L][2][k][n] in NTT form, the drop is one drop of fhe_mod_switch.  A plan holds G taps, 1 <= G <= 64: pairwise distinct Galois
 * elements g_j, odd, in [1, 2n) (g = 1: no rotation, no key), weights w_j, non-zero modulo t, with the centred lift w'_j in (-t/2, t/2]
 * reduced to every q_r (r < k), and K_j, the special Galois key for sigma_(g_j)(s) (a device pointer; ignored, and may be null, for g = 1).
 * With D_i,r = NTT_(q_r)([c_1,i]_(q_r)) ([.]_(q_r) as above: the integer in [0, q_i) reduced modulo q_r) and pi_g the permutation of NTT slots
 * with pi_g(NTT(a)) = NTT(sigma_g(a)) in R_(q_r):
 *   fhe_rotate_sum_sp:   acc_pp,r = sum_(j: g_j != 1) w'_j * sum_(i < L) pi_(g_j)(D_i,r) (*) K_j,i,pp,r  mod q_r   for every r < k,
 *                        u_pp = one drop (k -> k - 1) of acc_pp, bit for bit,
 *                        out_0 = u_0 + sum_j w'_j sigma_(g_j)(c_0),    out_1 = u_1 + sum_(j: g_j = 1) w'_j c_1;
 *   fhe_rotate_each_sp:  out[j] = (sigma_(g_j)(c_0) + u_0^(j), u_1^(j)), acc^(j) the inner sum of tap j alone (w' = 1); out[j] = ct for g_j = 1.
 *                        Output j of ciphertext c starts at out + j * tap_stride_words + c * out_stride_words.
 * All results are modulo q_r and fully reduced.  The digit of tap j is the integer polynomial sigma_(g_j)(d_i) taken over Z, coefficients in
 * (-q_i, q_i), reduced to every q_r: congruent to sigma_g(c_1) modulo q_i, so a valid RNS decomposition of the same magnitude.  It is NOT the
 * digit of fhe_apply_galois_sp, which negates modulo q_i and THEN reduces to q_r: the two differ by q_i mod q_r at every negated non-zero
 * coefficient for r != i, so these entry points decrypt to what the composition of fhe_apply_galois_sp, fhe_multiply_plain by the constant w_j
 * and fhe_add decrypts to, under the noise bound below, but their ciphertext bits are their own.
 * Noise: the call adds at most E = (sum_j |w'_j|) n B sum_(i < L) (q_i - 1) / p + (1 + n) / 2 to the numerator of the invariant noise (one
 * rounding, whatever G is) and scales the input's invariant noise by at most W = sum_j |w'_j|.  That factor IS the scalar products' usual
 * term: an integer scalar commutes with the scaling by t / Q up to multiples of t, so the (Q mod t) m / Q part of the input's invariant noise
 * grows with the rest of it and nothing is added beside it.  budget after >= -log2(W 2^-before + 2 t E / Q)  (circuits.rotate_sum_budget in
 * the Python host).
 * The slot permutations are derived, at plan creation, from the context's own forward transform of the monomial X (slot s holds psi^(e_s);
 * pi_g reads slot s from the slot holding psi^(e_s g mod 2n)): the NTT-form order stays internal.  weights == NULL: every weight is 1.  The plan keeps the key POINTERS: the keys must stay
 * where they are while the plan is used.  Plan creation allocates and synchronises; the two calls do neither.
 * In place: fhe_rotate_sum_sp allows out2 == ct2 with equal strides (the rule of fhe_apply_galois_sp); fhe_rotate_each_sp refuses any overlap.
 * Refused (FHE_ERR_PARAM) before anything is enqueued: k < 2, G == 0 or G > 64, an element that is even or >= 2n, a repeated element, a
 * weight that is 0 modulo t, a null key for g != 1, a null pointer, a stride below the ciphertext size (a tap stride below one batch of
 * outputs), scratch_bytes < fhe_rotsum_scratch_bytes(plan, count, each), a forbidden overlap.  count == 0 is a no-op. */
typedef struct fhe_rotsum_plan fhe_rotsum_plan;
int fhe_rotsum_plan_create(const fhe_ctx *ctx, uint32_t taps, const uint32_t *galois_elts, const uint64_t *weights,
                           const uint64_t *const *d_keys_ntt, fhe_rotsum_plan **out);
int fhe_rotsum_plan_destroy(fhe_rotsum_plan *plan);
size_t fhe_rotsum_scratch_bytes(const fhe_rotsum_plan *plan, uint64_t count, int each);
int fhe_rotate_sum_sp(const fhe_rotsum_plan *plan, const uint64_t *ct2, uint64_t ct_stride_words, uint64_t *out2, uint64_t out_stride_words,
                      uint64_t count, void *scratch, size_t scratch_bytes, fhe_stream stream);
int fhe_rotate_each_sp(const fhe_rotsum_plan *plan, const uint64_t *ct2, uint64_t ct_stride_words, uint64_t *out, uint64_t out_stride_words,
                       uint64_t tap_stride_words, uint64_t count, void *scratch, size_t scratch_bytes, fhe_stream stream);

/* ---- diagonal linear maps on the slots of ONE ciphertext under one special-prime key switch (csrc/rotdiag.hip) ------------------------------
 * fhe_rotate_sum_sp with a plaintext POLYNOMIAL per tap where it has one integer: out = sum_j p_j * rot_(g_j)(ct), the diagonal method's
 * sum_j d_j (.) rot_j(x) on the slots when p_j is the batch encoding of d_j.  Setting, level, key layout [L][2][k][n] and drop are those above.
 * A plan holds G taps, 1 <= G <= 64: pairwise distinct Galois elements g_j, odd, in [1, 2n) (g = 1: no rotation, no key), plaintexts p_j of n
 * coefficients modulo t, not the zero polynomial, with p'_j the centred lift (coefficients in (-t/2, t/2], reduced to every q_r: the lift of
 * fhe_multiply_plain), and K_j, the special Galois key for sigma_(g_j)(s) (may be null for g = 1).  With D_i,r and pi_g as above and
 * P_j,r = NTT_(q_r)(p'_j) in the context's own slot order:
 *   acc_pp,r = sum_(j: g_j != 1) P_j,r (*) sum_(i < L) pi_(g_j)(D_i,r) (*) K_j,i,pp,r  mod q_r   for every r < k,
 *   u_pp     = one drop (k -> k - 1) of acc_pp, bit for bit fhe_mod_switch's,
 *   out_0    = u_0 + sum_j p'_j sigma_(g_j)(c_0),    out_1 = u_1 + sum_(j: g_j = 1) p'_j c_1      (products in R_(q_r)).
 * All results are fully reduced.  The diagonal multiplies AFTER the rotation: tap j is multiply_plain(rotate(ct, g_j), p_j), and the result
 * decrypts to what that op-by-op composition decrypts to; its ciphertext bits are its own (the digit reason above).  When every p_j is a
 * constant polynomial w_j the definition is fhe_rotate_sum_sp's with the weights w_j: the same bytes.
 * Noise: fhe_rotate_sum_sp's bound with W = sum_j ||p'_j||_1 (circuits.rotate_diag_budget in the Python host).
 * plains_host [G][n] is HOST memory, read during plan creation only.  The plan keeps on the device the permutation tables, the key POINTER
 * table (the keys must stay where they are while the plan is used) and P [G][k][n], taken through the context's own forward transform, so
 * its slot order is that of D and of the keys on every path.  Plan creation allocates, launches and synchronises; the call does none of these.
 * In place: out2 == ct2 with equal strides is allowed; every other overlap is refused.
 * Refused (FHE_ERR_PARAM) before anything is enqueued: everything fhe_rotsum_plan_create / fhe_rotate_sum_sp refuse (the weight's check
 * becomes the plaintext's), a plaintext coefficient >= t, an all-zero plaintext, scratch_bytes < fhe_rotdiag_scratch_bytes(plan, count).
 * count == 0 is a no-op. */
typedef struct fhe_rotdiag_plan fhe_rotdiag_plan;
int fhe_rotdiag_plan_create(const fhe_ctx *ctx, uint32_t taps, const uint32_t *galois_elts, const uint64_t *plains_host,
                            const uint64_t *const *d_keys_ntt, fhe_rotdiag_plan **out);
int fhe_rotdiag_plan_destroy(fhe_rotdiag_plan *plan);
size_t fhe_rotdiag_scratch_bytes(const fhe_rotdiag_plan *plan, uint64_t count);
int fhe_rotate_diag_sum_sp(const fhe_rotdiag_plan *plan, const uint64_t *ct2, uint64_t ct_stride_words, uint64_t *out2, uint64_t out_stride_words,
                           uint64_t count, void *scratch, size_t scratch_bytes, fhe_stream stream);

/* ---- baby-step / giant-step linear maps on the slots of ONE ciphertext (csrc/rotbsgs.hip) --------------------------------------------------
 * out = sum_i rot_(h_i)( sum_j p_(i,j) * rot_(g_j)(ct) ): G1 G2 diagonals under G1 + G2 keys, where fhe_rotate_diag_sum_sp stops at 64 diagonals
 * and needs a key for each.  Setting, level, key layout [L][2][k][n], pi_g, the digit convention and the drop are those above.  A plan holds
 * G1 baby elements g_j and G2 giant elements h_i, 1 <= G1, G2 <= 64, each list odd, pairwise distinct and in [1, 2n) (1 is allowed in both
 * and needs no key), plaintexts p_(i,j) of n coefficients modulo t (plains_host [G2][G1][n]; an all-zero plaintext = the pair is ABSENT and
 * is skipped), and one special Galois key per non-identity baby element and per non-identity giant element.  With
 * P_(i,j),r = NTT_(q_r)(centred lift of p_(i,j)), D_l,r = NTT_(q_r)([c_1,l]_(q_r)), C0_r = NTT_(q_r)(c_0,r) and p the special prime:
 *   A(i)_pp,r = sum_(j present) P_(i,j),r (*) [ sum_(l < L) pi_(g_j)(D_l,r) (*) K_(g_j),l,pp,r                      (g_j != 1)
 *                                               + [pp = 0, r < L] [p]_(q_r) pi_(g_j)(C0_r) + [pp = 1, g_j = 1, r < L] [p]_(q_r) D_r,r ]  mod q_r
 *   v(i)      = one drop (k -> k - 1) of A(i)_1 for every i with h_i != 1, bit for bit fhe_mod_switch's, canonical coefficients,
 *   E(i)_l,r  = NTT_(q_r)([v(i)_l]_(q_r))   (the hoisted digit: the integer in [0, q_l) reduced to q_r, pi applied in NTT form),
 *   B_pp,r    = sum_(i: h_i != 1) [ sum_(l < L) pi_(h_i)(E(i)_l,r) (*) K_(h_i),l,pp,r + [pp = 0] pi_(h_i)(A(i)_0,r) ] + sum_(i: h_i = 1) A(i)_pp,r
 *               for every r < k (A(i)_0 is never dropped on its own: it is permuted and added at all k primes),
 *   out_pp    = one drop of B_pp, fully reduced.
 * With G2 = 1 and h = {1} the result is fhe_rotate_diag_sum_sp's bytes on the taps (g_j, p_(0,j)); with G1 = 1, g = {1}, p = the constant 1 and
 * one giant h != 1 it is fhe_rotate_sum_sp's bytes for the tap set {h} with weight 1.
 * Noise: circuits.rotate_bsgs_budget in the Python host: c_0 is rounded once, c_1 once per non-identity giant and once more.
 * plains_host is HOST memory, read during plan creation only.  The plan keeps on the device the permutation tables of both lists, the key
 * POINTER tables (the keys must stay where they are while the plan is used) and P for the present pairs only, taken through the context's
 * own forward transform.  Plan creation allocates, launches and synchronises; the call does none of these.
 * Scratch: fhe_rotbsgs_scratch_bytes(plan, count) = 8 count n ((L k + 3 k + 2) + G2 (2 k + 1 + L + L k)) bytes: fhe_rotdiag_scratch_bytes' and
 * per giant step A(i) [2][k][n], the special prime's row of A(i)_1 [n], v(i) [L][n] and E(i) [L][k][n].  Every giant step of every ciphertext
 * of the call is in flight at once; a caller short of memory splits the batch.
 * An identity giant step takes its row of v and E in the scratch and its share of the drop and digit launches although nothing reads them
 * (rows are not compacted): with G2 = 1 and h = {1} the call costs fhe_rotate_diag_sum_sp's work plus four launches and L k + L + 1
 * transforms per ciphertext -- use fhe_rotate_diag_sum_sp for that case.
 * The plan itself holds (pairs + 1) k n words on the device for `pairs` present pairs (plan creation stages the same amount on the host):
 * 64 MiB for 16 x 16 pairs and 1 GiB for a dense 64 x 64 plan at n = 8192, k = 4.
 * In place: out2 == ct2 with equal strides is allowed; every other overlap is refused.
 * Refused (FHE_ERR_PARAM) before anything is enqueued: everything fhe_rotdiag_plan_create / fhe_rotate_diag_sum_sp refuse, G1 or G2 of 0 or
 * above 64, a repeated element within a list, a giant step with no present pair, a baby step with no present pair (a key demanded for
 * nothing), a plaintext coefficient >= t, a null key for a non-identity element, scratch_bytes < fhe_rotbsgs_scratch_bytes(plan, count).
 * count == 0 is a no-op. */
typedef struct fhe_rotbsgs_plan fhe_rotbsgs_plan;
int fhe_rotbsgs_plan_create(const fhe_ctx *ctx, uint32_t G1, const uint32_t *baby_elts, uint32_t G2, const uint32_t *giant_elts,
                            const uint64_t *plains_host, const uint64_t *const *d_baby_keys_ntt, const uint64_t *const *d_giant_keys_ntt,
                            fhe_rotbsgs_plan **out);
int fhe_rotbsgs_plan_destroy(fhe_rotbsgs_plan *plan);
size_t fhe_rotbsgs_scratch_bytes(const fhe_rotbsgs_plan *plan, uint64_t count);
int fhe_rotate_bsgs_sp(const fhe_rotbsgs_plan *plan, const uint64_t *ct2, uint64_t ct_stride_words, uint64_t *out2, uint64_t out_stride_words,
                       uint64_t count, void *scratch, size_t scratch_bytes, fhe_stream stream);

/* ---- fused block circuit: encrypted_dct (homo/fhe_image.h:196-288) followed by quantize_fhe
 * (homo/fhe_image.h:294-305) on n_blocks independent 8x8 blocks.  in/out: [n_blocks][64][2][k][n].
 * The 832 Evaluator calls per block are exact operations in R_q, so the kernels transform each
 * input polynomial once, evaluate the whole linear circuit per NTT slot, and transform back:
 * the ciphertexts are bit-identical to the op-at-a-time evaluation.
 * quant64 == NULL builds a plan for encrypted_dct alone. */
int fhe_dct_plan_create(const fhe_ctx *ctx, const double *quant64, int int_coeffs, int frac_coeffs,
                        fhe_stream stream, fhe_dct_plan **out);
int fhe_dct_plan_destroy(fhe_dct_plan *plan);
/* scratch for fhe_dct8x8_quant: device memory of any 8-byte alignment.  The fused FP64 pair starts its intermediate at the
 * next multiple of 16 bytes inside it; the size returned includes those 16 bytes of slack (on every path). */
size_t fhe_dct8x8_scratch_bytes(const fhe_ctx *ctx, uint64_t n_blocks);
/* which kernels fhe_dct8x8_quant launches for this context (for labels in measurements): 1 = the fused exact-FP64
 * pair k_dct_rows + k_dct_cols (primes < 2^47, n <= 8192), 2 = the fused u64 pair k_dct_rows_u64 + k_dct_cols_u64
 * (primes <= 57 bits, n in 2048..8192), 0 = the general path k_ntt_fwd + k_dct_slots + k_ntt_inv. */
int fhe_dct_path(const fhe_ctx *ctx);
/* which arithmetic the u64 kernels of this context run on (for labels in measurements and for tests that must know which
 * kernels they exercised): bits 0-1 = class of the q-base, bits 2-3 = class of the auxiliary ct x ct base -- 0 Shoup / Harvey
 * kernels, 1 pseudo-Mersenne kernels for primes <= 55 bits, 2 pseudo-Mersenne kernels for primes <= 58 bits
 * (csrc/ntt_core.h) --, bit 4 = the ct x ct base conversions run as two-column sums (k_behz_to_bsk_pm,
 * k_behz_floor_back_pm).  0 when FHE_NTT_NOPM=1 was set at fhe_ctx_create or no prime of a base qualifies. */
int fhe_arith_path(const fhe_ctx *ctx);
int fhe_dct8x8_quant(const fhe_ctx *ctx, const fhe_dct_plan *plan, const uint64_t *in, uint64_t *out,
                     uint64_t n_blocks, void *scratch, size_t scratch_bytes, fhe_stream stream);

/* rgb_to_ycc_fhe (homo/fhe_image.h:310-325) on `count` pixels; r,g,b: [count][2][k][n], in place. */
int fhe_rgb_to_ycc(const fhe_ctx *ctx, uint64_t *r, uint64_t *g, uint64_t *b, uint64_t count,
                   int int_coeffs, int frac_coeffs, fhe_stream stream);
/* The same on the layout of the reference's ciphertext streams (homo/server_jpeg.cpp:115-124: per 8x8 block 64 R, 64 G,
 * 64 B ciphertexts): blocks [n_blocks][3][64][2][k][n], in place -> [n_blocks][Y, Cb, Cr][64][2][k][n], which read as
 * [3 n_blocks][64][2][k][n] is the input layout of fhe_dct8x8_quant and the order homo/server_jpeg.cpp:146-153 saves. */
int fhe_rgb_to_ycc_blocks(const fhe_ctx *ctx, uint64_t *blocks, uint64_t n_blocks, int int_coeffs, int frac_coeffs,
                          fhe_stream stream);

/* ---- the way back: dequantisation + 8x8 inverse DCT, and YCbCr -> RGB ------------------------------
 * fhe_idct8x8_dequant runs, on n_blocks independent 8x8 blocks of 64 size-2 ciphertexts c[0..63] (row-major),
 *     1. c[i] = multiply_plain(c[i], encode(Q[i]))          (skipped for a plan built with quant64 == NULL)
 *     2. idct_line(c[8r .. 8r+7]) for every row r
 *     3. idct_line(c[col], c[col+8], ..., c[col+56]) for every column col
 *     4. c[i] = multiply_plain(c[i], encode(0.125))
 * with encode = FractionalEncoder(int_coeffs, frac_coeffs) and idct_line the transpose of encrypted_dct's LL&M line
 * (IJG jidctint, the same twelve constants; A = add, S = sub, M = multiply_plain):
 *     z1 = M(A(d2, d6), .541196100);  t2 = A(z1, M(d6, -1.847759065));  t3 = A(z1, M(d2, .765366865))
 *     t0 = A(d0, d4);  t1 = S(d0, d4);  t10 = A(t0, t3);  t13 = S(t0, t3);  t11 = A(t1, t2);  t12 = S(t1, t2)
 *     u0, u1, u2, u3 = d7, d5, d3, d1;  z1 = A(u0, u3);  z2 = A(u1, u2);  z3 = A(u0, u2);  z4 = A(u1, u3)
 *     z5 = M(A(z3, z4), 1.175875602)
 *     u0 = M(u0, .298631336);  u1 = M(u1, 2.053119869);  u2 = M(u2, 3.072711026);  u3 = M(u3, 1.501321110)
 *     z1 = M(z1, -.899976223);  z2 = M(z2, -2.562915447)
 *     z3 = A(M(z3, -1.961570560), z5);  z4 = A(M(z4, -.390180644), z5)
 *     u0 = A(u0, A(z1, z3));  u1 = A(u1, A(z2, z4));  u2 = A(u2, A(z2, z3));  u3 = A(u3, A(z1, z4))
 *     out = [A(t10,u3), A(t11,u2), A(t12,u1), A(t13,u0), S(t13,u0), S(t12,u1), S(t11,u2), S(t10,u3)]
 * The result is bit-identical to that op-by-op sequence (steps 1 and 4 are applied as one product with the ring element
 * encode(Q[i]) * encode(0.125)).  in/out: [n_blocks][64][2][k][n]; out may alias in; n_blocks == 0 is a no-op; a zero
 * quant64[i] is refused.  Kernels as fhe_dct_path says: 1 = the fused exact-FP64 pair k_idct_rows + k_idct_cols, otherwise
 * k_ntt_fwd + k_idct_slots / k_idct_lines_pm + k_ntt_inv.  scratch: fhe_idct8x8_scratch_bytes (the fused pair's wave
 * intermediate, as fhe_dct8x8_quant's; 0 where the general path runs).
 * Plaintext growth: after fhe_dct8x8_quant, the chained products of fractional encodings pass t = 2^14 and wrap (the
 * decrypted pixels are wrong although the noise budget is large); a forward + inverse round trip needs t >= 2^22, and
 * t >= 2^26 with the colour conversion on both sides (rgb_to_ycc ... ycc_to_rgb). */
typedef struct fhe_idct_plan fhe_idct_plan;
int fhe_idct_plan_create(const fhe_ctx *ctx, const double *quant64, int int_coeffs, int frac_coeffs, fhe_stream stream,
                         fhe_idct_plan **out);
int fhe_idct_plan_destroy(fhe_idct_plan *plan);
size_t fhe_idct8x8_scratch_bytes(const fhe_ctx *ctx, uint64_t n_blocks);
int fhe_idct8x8_dequant(const fhe_ctx *ctx, const fhe_idct_plan *plan, const uint64_t *in, uint64_t *out,
                        uint64_t n_blocks, void *scratch, size_t scratch_bytes, fhe_stream stream);
/* JFIF YCbCr -> RGB, the inverse of rgb_to_ycc_fhe, on the stream layout: blocks [n_blocks][Y, Cb, Cr][64][2][k][n], in
 * place -> [n_blocks][R, G, B][64][2][k][n] (fhe_rgb_to_ycc_blocks' input layout):
 *     Y' = add_plain(Y, encode(128.0));  R = A(Y', M(Cr, 1.402));  G = S(S(Y', M(Cb, .344136)), M(Cr, .714136));  B = A(Y', M(Cb, 1.772))
 * bit-identical to that sequence; n_blocks == 0 is a no-op. */
int fhe_ycc_to_rgb_blocks(const fhe_ctx *ctx, uint64_t *blocks, uint64_t n_blocks, int int_coeffs, int frac_coeffs,
                          fhe_stream stream);

/* ---- 2-D convolution filters with public weights on encrypted pixels --------------------------------
 * Blur, sharpen, Sobel / Laplacian, the 2x2 average of 4:2:0 chroma subsampling: out[y][x] = sum_j,i w[j][i] * src[y sy + j - ay][x sx + i - ax]
 * on the per-pixel ciphertexts of the resize and decode streams.  Specification of ONE output ciphertext with tap indices
 * tap[0 .. kw*kh) (row-major over the kernel, x fastest) into a batch of source ciphertexts of `size` polynomials each:
 *     acc = none
 *     for p in 0 .. kw*kh - 1, in this order:
 *         if encode(w[p]) is the zero plaintext: continue         (SEAL 2.3 refuses multiply_plain by zero, and so does seal/seal.h)
 *         term = multiply_plain(src[tap[p]], encode(w[p]))        (encode = FractionalEncoder(int_coeffs, frac_coeffs, base 2))
 *         acc  = term if acc is none else add(acc, term)
 *     out = acc                                                   (`size` polynomials, fully reduced)
 * fhe_filter2d gives exactly these bits with ONE forward transform per source polynomial and ONE inverse transform per output
 * polynomial (csrc/filter.hip); taps that share a weight are summed before the product.  A kernel whose weights all encode to
 * zero, or a weight the encoder cannot hold, is refused by fhe_filter_plan_create.  Plaintext products only: no auxiliary base,
 * the ciphertext size stays what it was, every context fhe_ctx_create accepts is supported.
 *
 * Index arithmetic (host only; clamp-to-edge, the convention of fhe_resize_sample_plan): dst_w = ceil(src_w / stride_x),
 * dst_h = ceil(src_h / stride_y); output (x, y) reads source (clamp(x stride_x + i - anchor_x, 0, src_w - 1),
 * clamp(y stride_y + j - anchor_y, 0, src_h - 1)) for kernel position (i, j).  Streams interleave `channels` records per pixel: pixel
 * (x, y), channel c is record (y src_w + x) channels + c, and outputs come in the same interleaved order. */
#define FHE_FILTER_MAX_TAPS 64     /* kw * kh at most (7x7 and 8x8 kernels fit) */
typedef struct fhe_filter_plan fhe_filter_plan;
/* weights: [kh][kw] host doubles.  Each DISTINCT weight is encoded, lifted and transformed once and kept on the device. */
int fhe_filter_plan_create(const fhe_ctx *ctx, const double *weights, uint32_t kw, uint32_t kh, int int_coeffs, int frac_coeffs,
                           fhe_stream stream, fhe_filter_plan **out);
int fhe_filter_plan_destroy(fhe_filter_plan *plan);
/* number of kernel positions whose weight does not encode to zero */
int fhe_filter_plan_taps(const fhe_filter_plan *plan);
/* Host only, no context.  Writes [(row1 - row0) * dst_w * channels][kw * kh] record indices for destination rows [row0, row1), relative to
 * a resident window of source records that starts at source row src_row0 (which must not lie beyond the first row the shard
 * reads).  taps == NULL only reports dst_w and dst_h (the row arguments are then ignored).  0 <= anchor < kernel extent. */
int fhe_filter_tap_plan(uint32_t src_w, uint32_t src_h, uint32_t channels, uint32_t kw, uint32_t kh, int anchor_x, int anchor_y,
                        uint32_t stride_x, uint32_t stride_y, uint32_t row0, uint32_t row1, uint32_t src_row0, uint32_t *dst_w,
                        uint32_t *dst_h, uint32_t *taps);
/* The source rows destination rows [row0, row1) read (their own rows plus the halo, clamped): the counterpart of
 * fhe_resize_source_rows.  Destination rows are independent, so this is the multi-GPU partition: each device loads its rows plus
 * the halo and nothing is exchanged. */
int fhe_filter_source_rows(uint32_t src_h, uint32_t kh, int anchor_y, uint32_t stride_y, uint32_t row0, uint32_t row1, uint32_t *first,
                           uint32_t *count);
/* src: [n_src][size][k][n] device memory, never written.  out: [count][size][k][n], must not overlap src.  taps: HOST memory,
 * [count][kw * kh], consumed before the call returns.  src_is_ntt != 0: src already holds what fhe_ntt_forward writes (canonical
 * values), no forward pass runs and no scratch is needed -- a streaming server keeps its resident rows transformed and pays the
 * forward transform once per source row, not once per band.  Otherwise scratch holds the transformed sources
 * (fhe_filter2d_scratch_bytes = n_src * size * k * n * 8).  Everything is checked before anything is enqueued (a tap >= n_src,
 * size == 0, a plan of another context, short or overlapping scratch: FHE_ERR_PARAM).  count == 0 is a no-op. */
size_t fhe_filter2d_scratch_bytes(const fhe_ctx *ctx, const fhe_filter_plan *plan, uint32_t size, uint64_t n_src, uint64_t count,
                                  int src_is_ntt);
int fhe_filter2d(const fhe_ctx *ctx, const fhe_filter_plan *plan, const uint64_t *src, uint64_t n_src, uint32_t size, int src_is_ntt,
                 const uint32_t *taps, uint64_t *out, uint64_t count, void *scratch, size_t scratch_bytes, fhe_stream stream);
/* which kernels fhe_filter2d launches after the forward transforms (labels in measurements; tests that must know what they ran):
 * 1 / 2 = k_tap_sum_pm on the pseudo-Mersenne class 1 / 2 of the q-base (gather, lazy sums, products and the inverse transform
 * in one kernel), 0 = the general path k_tap_sum_mac + fhe_ntt_inverse on Shoup arithmetic, 4 = the general path with the transforms
 * on the exact-FP64 kernels (where fhe_ntt_forward runs them: n = 4096, primes <= 40 bits). */
int fhe_filter_path(const fhe_ctx *ctx);

/* ---- resampling with public weights on encrypted pixels: resize by any factor, rotate, warp ---------------
 * Where a pixel of the output lies in the source depends on the image dimensions (or the warp) alone, so the interpolation weights
 * are PUBLIC: resampling is a linear map with plaintext weights, multiply_plain and add only.  (The reference's SampleBicubic /
 * SampleLinear encrypt the offsets and multiply ciphertext by ciphertext: fhe_resize_bicubic_shared in include/fhe_circuits.h.)
 * fhe_remap is fhe_filter2d with the weights chosen PER OUTPUT.  A weight table holds the plaintexts; output o names, slot by slot, a
 * source ciphertext taps[o][p] and a table entry wids[o][p].  Specification of output o for tables of T slots per output:
 *     acc = none
 *     for p in 0 .. T - 1, in this order:
 *         if wids[o][p] == FHE_REMAP_SKIP or encode(w[wids[o][p]]) is the zero plaintext: continue
 *         term = multiply_plain(src[taps[o][p]], encode(w[wids[o][p]]))     (encode = FractionalEncoder(int_coeffs, frac_coeffs, base 2))
 *         acc  = term if acc is none else add(acc, term)
 *     out[o] = acc                                                          (`size` polynomials, fully reduced)
 * fhe_remap gives exactly these bits with ONE forward transform per source polynomial and ONE inverse transform per output polynomial
 * (csrc/resample.hip).  Plaintext products only: no auxiliary base, the ciphertext size stays what it was, every context
 * fhe_ctx_create accepts is supported.
 *
 * Weight table: each DISTINCT value (compared as doubles) is encoded, lifted and transformed once and kept on the device in the one
 * form the context's kernels read: k * n * 8 bytes per distinct entry on the pseudo-Mersenne paths (fhe_remap_path 1 / 2), k * n * 16
 * bytes (Shoup pairs) otherwise -- 256 KiB and 192 KiB per entry at P8192 and P4096.  Entries that encode to the zero plaintext take no
 * device memory and are remembered as such (their slots are skipped, as the specification says).  A value the encoder cannot hold, a
 * value that is not finite, count == 0 and more than FHE_REMAP_MAX_WEIGHTS distinct non-zero entries are refused.  A table belongs to
 * the context it was created with. */
#define FHE_REMAP_MAX_TAPS 64        /* slots per output */
#define FHE_REMAP_MAX_WEIGHTS 4096   /* distinct non-zero entries of one table (1 GiB at P8192) */
#define FHE_REMAP_SKIP 0xffffffffu   /* wids[o][p]: slot p of output o is unused */
typedef struct fhe_weight_table fhe_weight_table;
int fhe_weight_table_create(const fhe_ctx *ctx, const double *weights, uint32_t count, int int_coeffs, int frac_coeffs, fhe_stream stream,
                            fhe_weight_table **out);
int fhe_weight_table_destroy(fhe_weight_table *table);
/* entries (what wids index), and distinct entries held on the device */
int fhe_weight_table_count(const fhe_weight_table *table);
int fhe_weight_table_distinct(const fhe_weight_table *table);
/* src: [n_src][size][k][n] device memory, never written.  out: [count][size][k][n], must not overlap src.  taps, wids: HOST memory,
 * [count][T], consumed before the call returns; 1 <= T <= FHE_REMAP_MAX_TAPS.  src_is_ntt != 0: src already holds what fhe_ntt_forward
 * writes (canonical values), no forward pass runs and no scratch is needed; otherwise scratch holds the transformed sources
 * (fhe_remap_scratch_bytes = n_src * size * k * n * 8).  out_is_ntt != 0: the call stores the canonical slot-form sum -- exactly what
 * fhe_ntt_forward of the specified output would write -- and no inverse transform runs; a second fhe_remap takes that buffer with
 * src_is_ntt, so the two passes of a separable resize cost one transform pair per ciphertext, not two.  Everything is checked before
 * anything is enqueued, and a refused call writes nothing: an output without a live term (every slot skipped or a zero plaintext), a
 * tap >= n_src or a weight id >= fhe_weight_table_count in a slot that is not skipped, T out of range, size == 0, a table of another
 * context, out overlapping src, short or overlapping scratch: FHE_ERR_PARAM.  count == 0 is a no-op. */
size_t fhe_remap_scratch_bytes(const fhe_ctx *ctx, const fhe_weight_table *table, uint32_t size, uint64_t n_src, uint64_t count, int src_is_ntt);
int fhe_remap(const fhe_ctx *ctx, const fhe_weight_table *table, const uint64_t *src, uint64_t n_src, uint32_t size, int src_is_ntt,
              const uint32_t *taps, const uint32_t *wids, uint32_t T, uint64_t *out, int out_is_ntt, uint64_t count, void *scratch,
              size_t scratch_bytes, fhe_stream stream);
/* which kernels fhe_remap launches after the forward transforms: 1 / 2 = k_tap_sum_pm on the pseudo-Mersenne class 1 / 2 of the
 * q-base (gather, lazy sums, products and -- unless out_is_ntt -- the inverse transform in one kernel), 0 = the general path
 * k_tap_sum_mac (+ fhe_ntt_inverse) on Shoup arithmetic, 4 = the general path with the transforms on the exact-FP64 kernels. */
int fhe_remap_path(const fhe_ctx *ctx);

/* Index and weight arithmetic of ONE axis of a separable resize (host only, no context, callable without a device).  Writes
 * taps, weights: [dst_len][T]; both NULL only reports T.  Output x samples the source at u and reads T = 2 c consecutive positions
 * floor(u) - c + 1 .. floor(u) + c, clamped to the edge, c = ceil(radius * s): radius 1 (triangle), 2 (the cubics), 3 (Lanczos-3),
 * 1/2 (box); s = src_len / dst_len if antialias != 0 and src_len > dst_len (the kernel is stretched over the samples an output
 * covers), else 1.  The weight of position j is kernel((j - u) / s); the weights of one output are divided by their sum; with
 * weight_bits > 0 (at most 30) each is then rounded to a multiple of 2^-weight_bits (floor(w 2^bits + 1/2)) and what the sum lacks
 * to 1 is added to the largest (the first of equals), so the sum is exactly 1.  A plan of more than FHE_REMAP_MAX_TAPS taps is refused.
 * Kernels: TRIANGLE 1 - |d|;  CATMULL_ROM, the cubic of homo/fhe_resize.h:150-185 with a true t^3: weights (-t^3 + 2t^2 - t) / 2,
 * (3t^3 - 5t^2 + 2) / 2, (-3t^3 + 4t^2 + t) / 2, (t^3 - t^2) / 2 at offset t;  REFERENCE_CUBIC, the same polynomial with the
 * reference's t3 = t * t (:174-175): weights (t^2 - t) / 2, 1 - t^2, (t^2 + t) / 2, 0 -- what the ct x ct circuit computes;
 * LANCZOS3 sinc(d) sinc(d / 3) for |d| < 3;  BOX 1 on [-1/2, 1/2).
 * Conventions: HALF_PIXEL u = (x + 0.5) src_len / dst_len - 0.5 in double; with src_len == dst_len the plan is the identity, T = 1.
 * REFERENCE u = float(x) / float(dst_len - 1) * float(src_len) - 0.5 stored as float (homo/fhe_resize.h:351,382; dst_len >= 2),
 * first position int(u) - c + 1 (int() rounds towards zero, :228,260) and offset u - floor(u) (:230,262): the positions and offsets
 * of fhe_resize_sample_plan. */
#define FHE_RESAMPLE_TRIANGLE 0
#define FHE_RESAMPLE_CATMULL_ROM 1
#define FHE_RESAMPLE_REFERENCE_CUBIC 2
#define FHE_RESAMPLE_LANCZOS3 3
#define FHE_RESAMPLE_BOX 4
#define FHE_RESAMPLE_HALF_PIXEL 0
#define FHE_RESAMPLE_REFERENCE 1
int fhe_resample_axis_plan(uint32_t src_len, uint32_t dst_len, int kernel, int antialias, int convention, int weight_bits, uint32_t *T,
                           uint32_t *taps, double *weights);

/* ---- server-side encryptions (round 5) ------------------------------------------------------------
 * The reference's servers ENCRYPT inside their loops: SampleLinear / SampleBicubic encrypt frac(x) and frac(y) for every output
 * pixel (homo/fhe_resize.h:230,234,262,266: `encryptor.encrypt(encoder.encode(x - floor(x)), xfract)`), homomorphic_sin / cos an
 * encode(0) per call (homo/fhe_decode.h:54,134), server_decode the index and the accumulators (homo/server_decode.cpp:121,126).
 * With the circuits batched these encryptions were what a server spent its time on (host sampling, three uploads and five
 * launches per ciphertext); the entry points below form a whole batch on the device:
 *     Enc(m) = (Delta m' + pk0 u + e1, pk1 u + e2)        u ternary, e1, e2 rounded normals (sigma 3.19, redrawn beyond 19)
 * (textbook BFV, SURVEY.md App. A.7 -- what seal::Encryptor::encrypt computes; like every ciphertext of this build the bits are
 * the library's own: SEAL's sampler is not available here).
 *
 * Randomness: the ChaCha20 stream cipher (D. J. Bernstein's original layout: 256-bit key, 64-bit block counter, 64-bit nonce)
 * under a caller-supplied key.  Encryption number e = first_index + i of a key uses nonce e; 64-bit draw d of it is bytes
 * [8 d, 8 d + 8) of that stream (little endian): d = j for u_j, n + j for e1_j, 2 n + j for e2_j.  u_j = floor(3 r / 2^64) - 1;
 * the noise takes x = r >> 1, |e| = #{i : x >= cdt[i]} with cdt[i] = floor(2^63 P(|e| <= i)) (fhe_noise_cdt; integer work only,
 * so every implementation draws the same values), sign = low bit of r.  A (key, index) pair must never be used twice: draw the
 * key from the operating system's generator (getrandom) once per Encryptor and count.  tests/ pin the stream against the
 * published ChaCha20 vector, the table against a 90-digit evaluation, and the ciphertexts against the oracle's restatement. */
#define FHE_NOISE_CDT_LEN 19
void fhe_noise_cdt(uint64_t out[FHE_NOISE_CDT_LEN]);
/* FractionalEncoder::encode of `count` host doubles into d_plain [count][n] (device, coefficients below t): bit for bit
 * fhe_frac_encode of each value.  Asynchronous (the values travel through the staging ring). */
int fhe_frac_encode_batch(const fhe_ctx *ctx, const double *values, uint64_t count, int int_coeffs, int frac_coeffs,
                          uint64_t *d_plain, fhe_stream stream);
/* d_pk_ntt: the public key [2][k][n] in NTT form (fhe_ntt_forward of (pk0, pk1)); d_plain: [count][n] plaintext coefficients
 * below t, or NULL for encryptions of the zero plaintext; d_out: [count][2][k][n].  scratch: fhe_encrypt_scratch_bytes. */
size_t fhe_encrypt_scratch_bytes(const fhe_ctx *ctx, uint64_t count);
int fhe_encrypt_batch(const fhe_ctx *ctx, const uint64_t *d_pk_ntt, const uint64_t *d_plain, uint64_t count,
                      const uint8_t key[32], uint64_t first_index, uint64_t *d_out, void *scratch, size_t scratch_bytes,
                      fhe_stream stream);
/* the draws alone, for tests and for anyone who wants to check a ciphertext: d_draws [count][3][n] int8 (u, e1, e2) */
int fhe_encrypt_draws(const fhe_ctx *ctx, const uint8_t key[32], uint64_t first_index, uint64_t count, int8_t *d_draws,
                      fhe_stream stream);

/* ---- seeded symmetric encryption: fresh ciphertexts at half the bytes -------------------------------------------------
 * The client holds the secret key, so it can encrypt as (c0, c1) = (Delta m' - (a s + e), a) with a UNIFORM a expanded from a public
 * 32-byte a_key: only c0 and the key travel, the server regenerates a.  New entry points only (csrc/encrypt.hip).
 *   a:  ciphertext number e = first_index + i (wrapping modulo 2^64) is the ChaCha20 nonce under a_key (the cipher of fhe_encrypt_batch).
 *       For prime i and coefficient j, D = the 128-bit little-endian integer at bytes [16 (i n + j), 16 (i n + j) + 16) of that stream and
 *       a_i[j] = D mod q_i (bias below q_i / 2^128; no rejection, so the stream position never depends on the data).  Coefficient form.
 *       The residues of the first k' primes do not depend on k: the expansion in a level context is a prefix of the parent's.
 *   e:  the e1 draw of the sampler above under the SECRET noise_key: draws n .. 2 n - 1 of the stream (noise_key, nonce = e).
 *   c0 = Delta m' - (a s + e) with the lift of fhe_add_plain, so the phase c0 + c1 s is Delta m' - e in every residue.
 * An (a_key, index) pair must never be used twice under one secret key: two ciphertexts with the same a reveal the difference of their
 * plaintexts.  a_key is public and travels with the stream; noise_key never leaves the client.
 * Primes below 2^32 are refused (the 128-bit reduction needs 33 bits); the device pointers are 16-byte aligned.  Null pointers and a short
 * scratch are refused with the outputs untouched; count == 0 is a no-op.  Both work in a level context with sk[:k']. */
/* d_c0: [count][k][n] canonical residues; d_out: [count][2][k][n] (c0 copied into polynomial 0, a into polynomial 1); the ranges must not overlap */
int fhe_expand_seeded(const fhe_ctx *ctx, const uint64_t *d_c0, uint64_t count, const uint8_t a_key[32],
                      uint64_t first_index, uint64_t *d_out, fhe_stream stream);
/* c1 alone: d_a [count][k][n] (tests, and hosts that keep c0 elsewhere) */
int fhe_seed_expand_a(const fhe_ctx *ctx, uint64_t count, const uint8_t a_key[32], uint64_t first_index,
                      uint64_t *d_a, fhe_stream stream);
size_t fhe_encrypt_symmetric_scratch_bytes(const fhe_ctx *ctx, uint64_t count);
/* d_sk_ntt: [k][n] NTT form (what fhe_decrypt_batch takes); d_plain: [count][n] below t, or NULL for zero; d_c0: [count][k][n].
 * Refuses a batch whose index would wrap.  FHE_SYM_UNFUSED=1 (read at fhe_ctx_create) runs the composition of launches everywhere. */
int fhe_encrypt_symmetric_batch(const fhe_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_plain, uint64_t count,
                                const uint8_t a_key[32], const uint8_t noise_key[32], uint64_t first_index,
                                uint64_t *d_c0, void *scratch, size_t scratch_bytes, fhe_stream stream);

/* ---- decryption in batches (the clients' half: homo/client_jpeg.cpp:266-280, homo/client_resize.cpp:190-210) -----------------------
 * seal::Decryptor::decrypt of `count` ciphertexts of `size` polynomials: phase = sum_j c_j s^j (Horner per NTT slot), then
 * m = floor((t x + floor(q/2)) / q) mod t EXACTLY for x = the CRT value of the phase -- formed per coefficient from the residues with
 * multi-word integers on the device (no big-integer loop on the host).  d_sk_ntt: the secret key [k][n] in NTT form; d_ct:
 * [count][size][k][n]; d_plain: [count][n] coefficients below t; d_noise_bits (or NULL): [count] u32, the bit length of the largest
 * |t x - m q| of each ciphertext -- seal::Decryptor::invariant_noise_budget = max(0, fhe_ctx_modulus_bits - that - 1).
 * Bit for bit the oracle's big-integer decryption (tests/test_gpu_encrypt.py), also beyond the noise budget. */
uint32_t fhe_ctx_modulus_bits(const fhe_ctx *ctx);
size_t fhe_decrypt_scratch_bytes(const fhe_ctx *ctx, uint32_t size, uint64_t count);
int fhe_decrypt_batch(const fhe_ctx *ctx, const uint64_t *d_sk_ntt, const uint64_t *d_ct, uint32_t size, uint64_t count,
                      uint64_t *d_plain, uint32_t *d_noise_bits, void *scratch, size_t scratch_bytes, fhe_stream stream);

/* ---- synthetic inputs and digests (bench / parity harness) --------------------------------------
 * fill: value = splitmix64(seed ^ (first_linear_index + linear index)) mod q_i */
int fhe_fill_random(const fhe_ctx *ctx, uint64_t *ct, uint64_t n_polys, uint64_t seed,
                    uint64_t first_linear_index, fhe_stream stream);
/* order-independent 64-bit digest: sum over elements of splitmix64(value ^ splitmix64(index0+i))
 * mod 2^64, written to *d_out (device u64). */
int fhe_digest(const fhe_ctx *ctx, const uint64_t *data, uint64_t count, uint64_t index0,
               uint64_t *d_out, fhe_stream stream);

/* Input validation for ciphertext STREAMS (include/fhe_stream.h checks record headers only): ADDS to *d_count (device u64,
 * zeroed by the caller) the number of residues of the n_polys RNS polynomials at ct that are not below their modulus.
 * Every kernel assumes canonical residues -- seal::Ciphertext::load rejects anything else, and so does the facade's load --
 * so a server that takes streams from clients runs this on every wave it uploads (one HBM-bound pass, < 1 % of the PCIe
 * time of that wave) and refuses the job when the count is not zero.  homo/server_jpeg.cpp:117-123 is the load it guards. */
int fhe_count_unreduced(const fhe_ctx *ctx, const uint64_t *ct, uint64_t n_polys, uint64_t *d_count, fhe_stream stream);

#ifdef __cplusplus
}
#endif
#endif
