/*
 * lemsm -- MI355X (gfx950) MSM witness path for Liam Eagen's MSM argument.
 *
 * C ABI that the reference crate's Rust code would bind (see INTEGRATION.md for the
 * Rust `extern "C"` block and the shim that keeps the reference's entry signatures).
 * The reference has no FFI today; each entry below names the Rust function it stands
 * behind (paths relative to the reference repository root):
 *
 *   lemsm_msm_*                  halo2::arithmetic::best_multiexp(coeffs, bases)
 *                                (third-party; imported src/argument_witness_calc.rs:20,
 *                                called :144 and src/regular_functions_utils.rs:655,679,694,726)
 *   lemsm_lhs_msm_*              compute_lhs_witness MSM core, src/argument_witness_calc.rs:87-127,132-134
 *                                (the per-digit divisor witnesses of :129 stay in Rust; they are
 *                                built from the per-digit carries returned here)
 *   lemsm_negbase_decompose_batch negbase_decompose, src/negbase_utils.rs:20-36, over a slice
 *   lemsm_num_digits             d = logb_ceil(isqrt(order)+2, base)+1, src/argument_witness_calc.rs:89-91
 *   lemsm_precompute_multiplicities precompute_multiplicities, src/argument_witness_calc.rs:43-51
 *
 * Conventions
 *   scalars   n x 32 bytes, canonical little-endian integers < scalar-field order
 *             (== PrimeField::to_repr(), what best_multiexp and compute_lhs_witness read:
 *             src/argument_witness_calc.rs:93)
 *   field elt 4 x uint64 little-endian limbs in Montgomery form, R = 2^256
 *             (== SerdeObject::to_raw_bytes(), src/scripts.rs:44, src/precomputed_fft_data.rs:72)
 *   affine    (x[4], y[4]); the identity is (0,0)
 *   jacobian  (x[4], y[4], z[4]), x_aff = X/Z^2, y_aff = Y/Z^3; the identity has z == 0.
 *             Outputs are valid Jacobian points but their coordinates are NOT canonical
 *             (they depend on summation order); compare as group elements or through
 *             lemsm_jacobian_to_canonical.
 *   curves    LEMSM_BN254_G1: y^2 = x^3 + 3 over p, scalars mod r
 *             LEMSM_GRUMPKIN:  y^2 = x^3 - 17 over r, scalars mod p
 *
 * Ownership: the caller owns every buffer; the library neither keeps nor frees them.
 * Errors: non-zero lemsm_status; the reference's assert!/panic! sites map to
 *   LEMSM_ERR_LEN_MISMATCH (:88), LEMSM_ERR_SCALAR_OUT_OF_RANGE (:97, index in *bad_index),
 *   LEMSM_ERR_BAD_BASE (base < 3: the reference silently truncates for base 2).
 * Threading: a context is one GPU + one HIP stream + its workspace.  Calls on one context
 *   are serialised by the caller; different contexts may be used concurrently.  Every entry
 *   is synchronous: results are final on return.
 * There is no CPU fallback: without a usable gfx950 device lemsm_create fails.
 */
#ifndef LEMSM_H
#define LEMSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lemsm_ctx lemsm_ctx;

enum lemsm_curve { LEMSM_BN254_G1 = 0, LEMSM_GRUMPKIN = 1 };

enum lemsm_status {
  LEMSM_OK = 0,
  LEMSM_ERR_LEN_MISMATCH = 1,
  LEMSM_ERR_SCALAR_OUT_OF_RANGE = 2,
  LEMSM_ERR_BAD_BASE = 3,
  LEMSM_ERR_BAD_CURVE = 4,
  LEMSM_ERR_HIP = 5,
  LEMSM_ERR_BAD_ARG = 6,
  LEMSM_ERR_NOMEM = 7,
  LEMSM_ERR_TOO_MANY_DIGITS = 8,
  LEMSM_ERR_RCCL = 9,
  LEMSM_ERR_INDEX_OUT_OF_BOUNDS = 10,
  LEMSM_ERR_ARITH_OVERFLOW = 11,
  LEMSM_ERR_SUM_NOT_IDENTITY = 12,
  LEMSM_ERR_WOULD_NOT_TERMINATE = 13,
  LEMSM_ERR_DIVISION_BY_ZERO = 14,
  LEMSM_ERR_NOT_IN_TABLE = 15
};

/* ---- context ------------------------------------------------------------------------- */
/* Threading.  Any host thread may call any entry; a context is not tied to the thread that created it, and every entry
   is synchronous (results are final on return).  A context -- together with its host worker pool (option "host_threads"),
   its options (lemsm_set_option), its last_* state (lemsm_last_error, lemsm_last_bad_index, lemsm_last_truncated_count, the
   *_last telemetry getters) and the resident objects made through it (lemsm_device_alloc buffers, bases, fixed-base tables)
   -- serves ONE call at a time: the caller serialises the calls on one context, lemsm_destroy included; the pool is not
   reentrant.  Distinct contexts may be used concurrently from different threads, including several contexts on one
   device; lemsm_create / lemsm_destroy may run beside calls on other contexts.  Device pointers are only read by the
   entries that take them as inputs, so several contexts may read the same resident scalars / points at once.
   The contract is tested on the resident polynomial entries too (lemsm_fft* to lemsm_open_quotient*), their cached twiddle
   table, regrown workspaces, lemsm_poly_last / lemsm_sort_last and the error indices included.
   (tests/test_gpu_concurrency.py, tests/hostpool_race_check.cpp) */
int lemsm_create(int device, lemsm_ctx** out);
void lemsm_destroy(lemsm_ctx* ctx);
const char* lemsm_strerror(int status);
const char* lemsm_last_error(const lemsm_ctx* ctx);
/* index of the offending scalar after a LEMSM_ERR_SCALAR_OUT_OF_RANGE from an entry that has no
   bad_index parameter (lemsm_msm*: a scalar that is not a canonical field element) */
size_t lemsm_last_bad_index(const lemsm_ctx* ctx);
/* Number of scalars of the last negabase pass (lemsm_negbase_decompose_batch, lemsm_lhs_*) whose
   expansion needed more than d digits and was truncated exactly like the reference's
   `.chain(repeat(0)).take(d)` (src/argument_witness_calc.rs:99).  In-range scalars never truncate for
   base >= 3 with d = lemsm_num_digits; a non-zero count after a call with a smaller d
   means the digits no longer recompose the scalar. */
size_t lemsm_last_truncated_count(const lemsm_ctx* ctx);
/* Tuning / test knobs: "window_bits" (0 = auto), "chunk" (entries per accumulate thread,
   0 = auto), "tile" (pass-2 tile entries, 0 = auto), "binsort" (pass 2: 0/1 = bins of up to 36 864
   entries are bucket-sorted whole by one block, larger ones by the tiled kernels; 2 = tiled kernels only (A/B knob);
   > 2 = that capacity instead of 36 864, for tests that want both paths in one call), "field" (0 = lazy radix-2^29 arithmetic, the default;
   1 = strict 32-bit-limb arithmetic, kept for A/B and as an in-library cross-check),
   "accum_waves" (2..4 waves per SIMD of the accumulate kernel, 0 = auto), "groups" (window groups
   pipelined over three queues, device-pointer entries only; 0 = one group),
   "host_slab_bits" (host-pointer entries: log2 of the slab of pairs uploaded while the previous
   slab is being accumulated; 0 = auto = 21), "slab_bits" (device-pointer entries: log2 of the
   slab of pairs one pass of the pipeline covers; 0 = auto = 24, smaller values are a test knob),
   "merge_slice" (edge-record merge: pieces of a long bucket one wave adds, 0 = auto = 512; small values are a
   test knob), "merge_wave_th" (buckets of 9..32 pieces get one wave each while there are fewer than this many,
   0 = auto = 2049; 1 = always serial),
   "abi_points" (lazy arithmetic: 1 = convert the points to the kernels' domain in a pass of their
   own, 2 = let the accumulation consume them as passed in, 0 = choose by segment length and window
   count), "pyr_fuse" (bucket-reduction pyramid: 0 = one launch per step while a window's step has more than 256 items, the
   rest in one launch of one block per window; 1 = one launch per step throughout; 2 = fuse from 2048 items: A/B knob), "host_threads" (host tail: 0 = up to 8 threads, 1 = serial), "pyr_first2" (1 = the first two pyramid steps in one pass over the bucket sums where the window has
   >= 32 buckets -- half the HBM traffic of the two launches, measured no faster: A/B knob; 0 = one launch per step), "ntt_tiled" (divisor witness: 0 = LDS-tiled transforms, up to 10 stages per launch; 2 = one launch per
   stage: A/B knob), "dw_kb" (divisor witness: slots per thread of the batched-inversion kernels, 8..64; 0 = auto),
   "dw_fuse" (divisor witness: 0 = the first forward transform pass of a level gathers its
   input from the coefficient arrays and the last inverse pass scatters into them; 2 = separate load / store kernels:
   A/B knob), "dw_pw_lazy" (divisor witness: 1 = the pointwise numerators in the lazy 29-bit field -- 12 cheaper products, paid back by the
   conversions around them: measured no faster; 0 = strict field: A/B knob), "scatter_lean" (pass 1 of the bucket sort: 1 = a thread of k_scatter1 owns two adjacent bins, one block scan, unrolled store loop -- measured no faster, profiles/r03/s_scatter_lean_and_clear_beside_ab.txt; 0 = bins tid and tid + 256: A/B knob), "scatter_tile" (pass 1 of the bucket sort, Pippenger digits: 0 = auto -- whole 32768-scalar tiles per 1024-thread block that claim their runs in-kernel (k_scatter_tile) where
   windows x tiles fill the chip several times over, k_scatter1 over 4096-scalar ranges otherwise; 1 = tiles wherever the decoder allows it, whatever n: test knob; 2 = never), "pyr_quad" (bucket-reduction pyramid, lazy arithmetic: 0 = steps that leave most of the chip without a wave -- and the fused last steps -- run four lanes per addition (one product per lane and stage, DPP quad exchanges: ~2.6x shallower); 2 = one lane per addition: A/B knob), "slab_tail" (calls of more than one slab of points -- more than 2^24, or option slab_bits: 0 = every slab accumulates into a bucket area of its own and the call runs one bucket reduction and leaves one block of records (up to 8 slabs); 2 = a reduction per slab, the records added on the host: A/B knob), "dw_halves" (divisor witness: 1 = the pointwise chain of a level runs as two halves of its nodes on two queues, one half's batched inversion beside the other half's numerators: measured no faster, profiles/r03/k_halves_trace.txt; 0 = one chain: A/B knob), "dw_ntt_lazy" (divisor witness: 1 = the butterflies of the LDS-tiled transforms in the lazy 29-bit field, twiddles from a second table -- measured 1 % slower: the strict product is 128 multiply-adds here, the lazy one 162 plus carry passes; 0 = strict field: A/B knob), "dw_reuse" (divisor witness: 0 = a level transforms its children onto the odd half of its domain only and reads the even half from the level
   below's evaluations, 2 = whole transforms: A/B knob), "dw_wrap" (divisor witness: 0 = levels whose longest part
   has 2^k + 1 coefficients run on 2^k-point transforms, the folded top coefficient recovered from the value at x = 0;
   2 = always the next power of two: A/B knob), "ws_canary" (1 = debug: every sub-buffer of the MSM workspace is followed by a 256-byte guard that is
   filled before and verified after every window group; an overrun returns LEMSM_ERR_HIP naming the guard; the fuzz
   soak turns it on at random), "validate_points" (1: lemsm_msm*, lemsm_lhs_msm* check y^2 = x^3 + b for every non-identity input point
   before any work and return LEMSM_ERR_BAD_ARG with the index in lemsm_last_bad_index; 0, the default, trusts the
   caller like the reference's from_raw_bytes_unchecked does -- the hot kernel tests y alone for the identity,
   so an invalid (x != 0, y == 0) input would otherwise be skipped silently), "open_group" (lemsm_poly_lincomb* /
   lemsm_open_quotient*: terms of the combination that share one Montgomery reduction, 1 .. 5; 0 = 5, the most one
   conditional subtraction allows; 1 = a reduction per term: A/B knob, the bytes do not depend on it). */
int lemsm_set_option(lemsm_ctx* ctx, const char* name, long value);
/* Device-time (ms, from HIP events on the context's stream) of the last MSM call: whole
   pipeline in [0], the dominant accumulate kernel in [1], its launch count in [2]. */
int lemsm_last_timing(const lemsm_ctx* ctx, double out[3]);
/* Shader clock (MHz) the accumulate kernel of the last MSM call sustained, from in-kernel stamps
   (s_memtime / s_memrealtime around one mid-grid wave's whole chunk); 0 if no launch stamped. */
int lemsm_last_accum_clock_mhz(const lemsm_ctx* ctx, double* out);
/* Test / profiling aid: how the edge-record merge of the last MSM call classified the buckets that straddle
   accumulate chunks, summed over window groups and slabs: [0] 3..8 pieces (serial), [1] 9..32 pieces,
   [2] slices of buckets of more than 32 pieces, [3] buckets of several slices.  Two-piece buckets are not counted. */
int lemsm_debug_last_merge_counts(const lemsm_ctx* ctx, uint64_t out[4]);

/* ---- best_multiexp ------------------------------------------------------------------- */
/* sum_i scalars[i] * points[i]; host buffers. */
int lemsm_msm(lemsm_ctx* ctx, int curve, const uint8_t* scalars, const uint64_t* points_affine,
              size_t n, uint64_t out_jacobian[12]);
/* `batch` MSMs over the same points: sum_i scalars_k[i] * points[i] for k < batch; d_scalars[k]: device pointer to n x 32 B,
   outs: batch x 12 limbs.  The calls are pipelined over two lanes of queues and workspaces: the host tail of call k - 1 and
   its latency-bound bucket-reduction tail overlap call k's passes (a prover calls best_multiexp many times over one SRS:
   /root/reference/src/argument_witness_calc.rs:144, src/regular_functions_utils.rs:655-726).  Results equal `batch`
   separate lemsm_msm_device calls; the first failing call's status is returned. */
int lemsm_msm_batch_device(lemsm_ctx* ctx, int curve, const void* const* d_scalars, size_t batch, const void* d_points_affine,
                           size_t n, uint64_t* outs);
int lemsm_msm_bn254_g1(lemsm_ctx* ctx, const uint8_t* scalars, const uint64_t* points_affine,
                       size_t n, uint64_t out_jacobian[12]);
int lemsm_msm_grumpkin(lemsm_ctx* ctx, const uint8_t* scalars, const uint64_t* points_affine,
                       size_t n, uint64_t out_jacobian[12]);
/* Same with inputs already resident in this context's GPU memory (device pointers). */
int lemsm_msm_device(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine,
                     size_t n, uint64_t out_jacobian[12]);

/* Window-sharded form (multi-GPU: each rank computes a range of Pippenger windows, ranks
   exchange the small partial records, everyone combines).  lemsm_msm_plan reports the number
   of windows and the byte size of one window's partial record for an n-point MSM: the record is
   the window's sum S_w = sum_k k * Bucket_{w,k} as one XYZZ point (x, y, zz, zzz; 4 x 32 bytes raw
   Montgomery; zz == 0 is the identity). */
int lemsm_msm_plan(const lemsm_ctx* ctx, int curve, size_t n, uint32_t* num_windows,
                   size_t* partial_bytes_per_window);
int lemsm_msm_partial_device(lemsm_ctx* ctx, int curve, const void* d_scalars,
                             const void* d_points_affine, size_t n, uint32_t win_begin,
                             uint32_t win_end, uint8_t* out_partials /* (win_end-win_begin) records */);
int lemsm_msm_combine(const lemsm_ctx* ctx, int curve, size_t n, const uint8_t* partials_all_windows,
                      uint64_t out_jacobian[12]);

/* ---- multi-GPU: Pippenger-window sharding over the GPUs of one node, RCCL over xGMI ------ */
/* The reference has no distributed code (its parallelism is Rayon inside best_multiexp, called at
   src/argument_witness_calc.rs:144); these entries are what its Rust host binds to use more than one GPU.
   Rank r of G owns windows [W r / G, W (r+1) / G) (digit positions on the lhs path) over ALL points, which every rank
   holds in its own HBM; the ranks exchange the raw per-window records with ONE ncclAllGather straight from device
   memory (EC addition is not an RCCL reduction operator) and every rank combines, so every rank returns the
   same group element.  RCCL is bound at run time (dlopen of librccl.so.1; override with LEMSM_RCCL_LIB): the
   single-GPU entries never need it, a failure to load it is LEMSM_ERR_RCCL here.
   Two ways in:
     one process per GPU   lemsm_comm_unique_id on rank 0, the 128 bytes sent to the other ranks by the host's own
                           means, lemsm_comm_init on every rank (collective), then lemsm_*_sharded_device (collective);
     one process, N GPUs   lemsm_node_*: contexts, communicators and one host thread per GPU inside the library. */
#define LEMSM_COMM_ID_BYTES 128
int lemsm_comm_unique_id(uint8_t id[LEMSM_COMM_ID_BYTES]);
int lemsm_comm_init(lemsm_ctx* ctx, const uint8_t id[LEMSM_COMM_ID_BYTES], int nranks, int rank);
int lemsm_comm_destroy(lemsm_ctx* ctx);
int lemsm_comm_info(const lemsm_ctx* ctx, int* nranks, int* rank);   /* nranks = 0: no communicator */
/* Collective over the context's communicator; inputs resident on every rank.  With automatic window width a
   sharded call uses 16-bit windows from 2^24 points (16 windows split evenly over 2/4/8 ranks). */
int lemsm_msm_sharded_device(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine, size_t n,
                             uint64_t out_jacobian[12]);
int lemsm_lhs_msm_sharded_device(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine, size_t n,
                                 uint8_t base, uint64_t out_carry[12], uint64_t* out_carries, size_t* bad_index);

typedef struct lemsm_node lemsm_node;
/* devices == NULL: devices 0..ndev-1 */
int lemsm_node_create(const int* devices, int ndev, lemsm_node** out);
void lemsm_node_destroy(lemsm_node* node);
int lemsm_node_size(const lemsm_node* node);
lemsm_ctx* lemsm_node_ctx(lemsm_node* node, int i);
const char* lemsm_node_last_error(const lemsm_node* node);
/* bases: n affine points (host), replicated into every GPU once and kept resident (halo2's bases are a fixed SRS) */
int lemsm_node_set_bases(lemsm_node* node, int curve, const uint64_t* points_affine, size_t n);
/* best_multiexp(scalars, bases[..n]) over the node.  Every GPU uploads one G-th of the scalar vector over its own PCIe link and
   an in-place all-gather over xGMI completes the copies (the host's memory is read once, not G times). */
int lemsm_node_msm(lemsm_node* node, const uint8_t* scalars, size_t n, uint64_t out_jacobian[12]);
/* compute_lhs_witness MSM core over the node (n must equal the number of resident bases, :88) */
int lemsm_node_lhs_msm(lemsm_node* node, const uint8_t* scalars, size_t n, uint8_t base, uint64_t out_carry[12],
                       uint64_t* out_carries, size_t* bad_index);

/* ---- resident bases on one GPU ------------------------------------------------------- */
/* best_multiexp(&scalars, &pts_aff) (src/argument_witness_calc.rs:144) with pts_aff uploaded once: later calls move
   only the scalars over PCIe, slab by slab under the kernels of the previous slab. */
typedef struct lemsm_bases lemsm_bases;
int lemsm_bases_upload(lemsm_ctx* ctx, int curve, const uint64_t* points_affine, size_t n, lemsm_bases** out);
void lemsm_bases_free(lemsm_bases* bases);
const void* lemsm_bases_device_ptr(const lemsm_bases* bases);
int lemsm_msm_with_bases(lemsm_ctx* ctx, const lemsm_bases* bases, const uint8_t* scalars, size_t n, uint64_t out_jacobian[12]);
/* `batch` MSMs over the same resident bases with the scalar vectors in host memory (scalars[k]: n x 32 B; outs: batch x 12 limbs):
   the upload of call k's scalars and the host fold of call k - 1 run while the GPU works on the neighbouring call, so a call costs
   the longer of upload and compute, not their sum (how a prover calls best_multiexp over one SRS:
   /root/reference/src/argument_witness_calc.rs:144).  Results equal `batch` lemsm_msm_with_bases calls; the first failing
   call's status is returned. */
int lemsm_msm_batch_with_bases(lemsm_ctx* ctx, const lemsm_bases* bases, const uint8_t* const* scalars, size_t batch, size_t n, uint64_t* outs);

/* ---- fixed-base MSM: precomputed window tables over resident bases --------------------- */
/* best_multiexp(&scalars, &pts_aff) (src/argument_witness_calc.rs:144) for a prover that calls it many times over one SRS.
   A table holds m shifted copies T_k[i] = 2^(c h k) P_i of the bases (k < m, h = ceil(W / m), W signed c-bit windows whose
   top digit stays below 2^(c-1)), row i * m + k, 64 B each in the ABI's affine form (identity: all-zero row).  A call runs
   the bucket pipeline over n * m "virtual points" with h windows that all m tables share: one bucket set and one pyramid
   per folded window, the host's Horner over h windows only (none at h = 1).  Geometry: c in [3, 17], m in [1, W]; 0 = auto
   (a cost model: n W accumulate additions, 2 h 2^(c-1) pyramid additions, a fixed cost per slab of 2^24 virtual points;
   an automatic plan keeps its table within 16 GiB).  Out of scope: multi-GPU, batch entries and the negabase path. */
typedef struct lemsm_fixed_bases lemsm_fixed_bases;
/* Pure host: the geometry a table over n bases would get (window_bits / tables 0 = auto); device_bytes = m * n * 64.
   LEMSM_ERR_BAD_ARG for a window width outside [3, 17] or more tables than windows.  (best_multiexp, :144) */
int lemsm_fixed_plan(int curve, size_t n, uint32_t window_bits, uint32_t tables, uint32_t* c, uint32_t* num_windows, uint32_t* m,
                     uint32_t* h, size_t* device_bytes);
/* Builds the table of `bases` on the context's GPU (one doubling chain per base and table, one inversion per base).
   LEMSM_ERR_NOMEM, before any kernel runs, when the table does not fit in free device memory.  Free the table before its
   context is destroyed, like lemsm_bases; the bases themselves may be freed once the table exists.  (best_multiexp, :144) */
int lemsm_fixed_bases_create(lemsm_ctx* ctx, const lemsm_bases* bases, uint32_t window_bits, uint32_t tables,
                             lemsm_fixed_bases** out);
/* The table's geometry (as lemsm_fixed_plan).  (best_multiexp, :144) */
int lemsm_fixed_bases_info(const lemsm_fixed_bases* fb, uint32_t* c, uint32_t* num_windows, uint32_t* m, uint32_t* h,
                           size_t* device_bytes);
/* the table on the device: row i * m + k = 2^(c h k) bases[i] (64 B, affine ABI form) */
const void* lemsm_fixed_bases_device_ptr(const lemsm_fixed_bases* fb);
void lemsm_fixed_bases_free(lemsm_fixed_bases* fb);
/* best_multiexp(scalars, bases[0..n]) (:144) for n <= the table's n (halo2 commits to prefixes of the SRS).  Result and status
   codes are those of lemsm_msm: a non-canonical scalar is LEMSM_ERR_SCALAR_OUT_OF_RANGE with its index in
   lemsm_last_bad_index, n above the table's n is LEMSM_ERR_LEN_MISMATCH, a table of another context LEMSM_ERR_BAD_ARG. */
int lemsm_msm_fixed(lemsm_ctx* ctx, const lemsm_fixed_bases* fb, const uint8_t* scalars, size_t n, uint64_t out_jacobian[12]);
/* the same with the scalars already on the context's GPU (n x 32 B) */
int lemsm_msm_fixed_device(lemsm_ctx* ctx, const lemsm_fixed_bases* fb, const void* d_scalars, size_t n, uint64_t out_jacobian[12]);

/* ---- negabase decomposition ---------------------------------------------------------- */
int lemsm_num_digits(int curve, uint8_t base, uint32_t* d);
/* digits[i*d + k] = k-th negabase digit (LSB first, in [0,base)) of scalar i, zero padded /
   truncated to d exactly like `.chain(repeat(0)).take(d)` (src/argument_witness_calc.rs:99). */
int lemsm_negbase_decompose_batch(lemsm_ctx* ctx, const uint8_t* scalars, size_t n, uint8_t base,
                                  uint32_t d, uint8_t* digits);

/* ---- prepare_scalar_witness / table_entry_by_id -------------------------------------- */
/* prepare_scalar_witness(sc, base, num_digits, logtable), src/negbase_utils.rs:79-124, for each of n scalars, computed
   exactly as the reference's code does (limb index i % logtable + 1, :98-101 -- not upstream's presumable intent).
   scalars: n x 32 bytes little-endian magnitudes; negative: optional n flags (the reference takes a signed BigInt).
   out_entries: n x base x (num_limbs+1) entries, num_limbs = ceil(num_digits / logtable), row-major like the returned
   Vec<Vec<Entry>>; one entry = 24 bytes {int128 value (two's complement LE), uint32 mask, uint32 kind} with
   kind 0 = Entry::Scalar (value: the scalar's low 128 bits), 1 = Entry::Bucket(value), 2 = Entry::Limb(value, mask).
   Where the reference would panic the first offending scalar's index goes to *bad_index and the status says why:
   LEMSM_ERR_TOO_MANY_DIGITS (assert :81), LEMSM_ERR_INDEX_OUT_OF_BOUNDS (:98-101 when i % logtable + 1 > num_limbs),
   LEMSM_ERR_ARITH_OVERFLOW (pow / += overflow of i128 or u32, :97-101: a panic in the reference's debug build). */
int lemsm_prepare_scalar_witness_batch(lemsm_ctx* ctx, const uint8_t* scalars, const uint8_t* negative, size_t n,
                                       uint8_t base, uint32_t num_digits, uint32_t logtable, uint8_t* out_entries,
                                       size_t* bad_index);
/* table_entry_by_id(base, id), src/negbase_utils.rs:58-77, for id in [id_begin, id_begin + count), in the BASE field of
   `curve` (the circuit's native field: C::Base, src/config.rs:486); out: count x 4 limbs raw Montgomery.
   As the reference computes it: sum over the set bits k of id of (-base)^(k+1). */
int lemsm_table_entries(lemsm_ctx* ctx, int curve, uint8_t base, uint64_t id_begin, size_t count, uint64_t* out);

/* ---- compute_lhs_witness MSM core ---------------------------------------------------- */
/* carry = sum_j scalars[j]*pts[j] via the Horner-in-(-base) recursion over negabase digits.
   out_carries (optional, d x 12 limbs): carry after each digit position, MSB first -- the
   value the reference negates and pushes at :127.  Scalars must be < isqrt(order)+2 (:97). */
int lemsm_lhs_msm(lemsm_ctx* ctx, int curve, const uint8_t* scalars, const uint64_t* pts_jacobian,
                  size_t n, uint8_t base, uint64_t out_carry[12], uint64_t* out_carries,
                  size_t* bad_index);
int lemsm_lhs_msm_grumpkin(lemsm_ctx* ctx, const uint8_t* scalars, const uint64_t* pts_jacobian,
                           size_t n, uint8_t base, uint64_t out_carry[12], uint64_t* out_carries,
                           size_t* bad_index);
int lemsm_lhs_msm_bn254_g1(lemsm_ctx* ctx, const uint8_t* scalars, const uint64_t* pts_jacobian,
                           size_t n, uint8_t base, uint64_t out_carry[12], uint64_t* out_carries,
                           size_t* bad_index);
/* Device-resident form; points already affine (n x 8 limbs). */
int lemsm_lhs_msm_device(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine,
                         size_t n, uint8_t base, uint64_t out_carry[12], uint64_t* out_carries,
                         size_t* bad_index);
/* Digit-position-sharded form for multi-GPU. */
int lemsm_lhs_plan(int curve, uint8_t base, uint32_t* num_positions, size_t* partial_bytes_per_position);
int lemsm_lhs_partial_device(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine,
                             size_t n, uint8_t base, uint32_t pos_begin, uint32_t pos_end,
                             uint8_t* out_partials, size_t* bad_index);
int lemsm_lhs_combine(int curve, uint8_t base, const uint8_t* partials_all_positions,
                      uint64_t out_carry[12], uint64_t* out_carries);

/* ---- divisor witness (the second return value of compute_lhs_witness) ----------------- */
/* compute_divisor_witness_partial / compute_divisor_witness (src/regular_functions_utils.rs:453-480): the regular function
   a(x) + y b(x) vanishing on the n points and on minus their sum, built by the reference's pairwise merge tree
   (Propagation::group_merge :380-405) -- every level one GPU batch: NTTs over bn256::Fr, pointwise products with
   y^2 = x^3 - 17 substituted (:266-273), the two exact divisions of merge (:357) done in the evaluation domain.
   Grumpkin only (C::Base: FftPrecomp, src/precomputed_fft_data.rs:3).  points: n affine points, identity = (0,0).
   out_a / out_b: coefficients, 4 raw-Montgomery limbs each, constant term first; *len_a / *len_b: the reference's vector
   lengths exactly (trailing zero coefficients it carries included); n + 2 coefficients per part always suffice.
   normalise != 0: scaled so that the coefficient of highest pole order (x^i: 2i, y x^i: 2i + 3) is 1.  A witness is only
   defined up to a scalar (linefunc works on whatever projective representative a point has, :285-303, :426-431): the
   normalised form is the representation-independent one.
   require_zero_sum != 0: LEMSM_ERR_SUM_NOT_IDENTITY when the points do not sum to the identity (panic at :478).
   out_point_affine (optional): the tree's output = minus the sum of the points (the `.1` of _partial).
   LEMSM_ERR_ARITH_OVERFLOW: two empty polynomials meet in a product (usize underflow at :55, a panic in the reference:
   four identity points in an aligned group of four).
   LEMSM_ERR_BAD_ARG when cap_a < *len_a or cap_b < *len_b: both lengths are set, out_a and out_b are untouched and no
   work of the call is left queued. */
int lemsm_divisor_witness(lemsm_ctx* ctx, int curve, const uint64_t* points_affine, size_t n, int require_zero_sum,
                          int normalise, uint64_t* out_a, size_t cap_a, size_t* len_a, uint64_t* out_b, size_t cap_b,
                          size_t* len_b, uint64_t out_point_affine[8]);
int lemsm_divisor_witness_device(lemsm_ctx* ctx, int curve, const void* d_points_affine, size_t n, int require_zero_sum,
                                 int normalise, uint64_t* out_a, size_t cap_a, size_t* len_a, uint64_t* out_b,
                                 size_t cap_b, size_t* len_b, uint64_t out_point_affine[8]);
/* T independent point lists in ONE batch (the merge trees of all lists advance level by level together: the launch
   count of a single tree).  list t = counts[t] affine points, lists concatenated.  out_index: T x 4 entries
   {offset_a, len_a, offset_b, len_b} in elements of 4 limbs into out_coeffs (a list of n points gives n + 1 coefficients in
   all unless identities or P / -P pairs make the reference carry zero padding: 2 sum(counts) + 4 T elements always suffice);
   out_points_affine (optional): T x 8 limbs.  With require_zero_sum the first offending list is in lemsm_last_bad_index.
   LEMSM_ERR_BAD_ARG when cap_coeffs is too small: out_index then holds the complete layout (the elements the call needs
   are offset_b + len_b of its last row), out_coeffs is untouched and no work of the call is left queued. */
int lemsm_divisor_witness_batch(lemsm_ctx* ctx, int curve, const uint64_t* points_affine, const size_t* counts, size_t T,
                                int require_zero_sum, int normalise, uint64_t* out_coeffs, size_t cap_coeffs,
                                size_t* out_index, uint64_t* out_points_affine);
/* Test / profiling aid: levels of the last divisor-witness forest whose forward transforms covered only the odd half of the
   level's domain, the even half being the level below's own evaluations (child-evaluation reuse; option "dw_reuse" 2 = off). */
int lemsm_debug_divisor_last_reuse_levels(const lemsm_ctx* ctx, uint32_t* levels);
/* Device time (ms) of the transform launches of the last divisor-witness call (with option dw_fuse at its default the
   first forward and the last inverse pass of a level also gather from / scatter into the coefficient arrays), their algorithmic bytes (every element
   read once and written once per pass over HBM: 1 pass up to 2^10 elements, 2 up to 2^18, 3 beyond) and their butterfly
   count (one field multiplication each): the figures the HBM and VALU rooflines of the transforms are priced with. */
int lemsm_divisor_last_ntt(const lemsm_ctx* ctx, double* ms, uint64_t* algorithmic_bytes, uint64_t* butterflies);
/* compute_lhs_witness in full (src/argument_witness_calc.rs:87-136): carry = sum_j scalars[j] pts[j] AND the d divisor
   witnesses of :129 (function f = digit iteration d - 1 - f, the reference's `ret.reverse()` order).
   out_coeffs: cap_coeffs field elements (4 limbs each); out_index: d x 4 entries {offset_a, len_a, offset_b, len_b} in
   elements; a function over a list of c points has c + 1 coefficients in all (up to 2 c + 2 when identities or
   opposite points make the reference carry zero padding): 2 d (n + base + 3) elements always suffice.
   LEMSM_ERR_BAD_ARG when cap_coeffs is too small (this entry, _device and _device_range alike): out_carry and the
   complete out_index are set (the elements the call needs are offset_b + len_b of its last row), out_coeffs is
   untouched -- nothing has been copied into it -- and no work of the call is left queued. */
int lemsm_lhs_witness(lemsm_ctx* ctx, int curve, const uint8_t* scalars, const uint64_t* pts_jacobian, size_t n,
                      uint8_t base, uint64_t out_carry[12], uint64_t* out_coeffs, size_t cap_coeffs, size_t* out_index,
                      int normalise, size_t* bad_index);
/* The same with the scalars and the AFFINE points (64-byte rows, as the device-pointer MSM entries take them) already in
   HBM and the coefficients left in HBM (d_out_coeffs: device buffer of cap_coeffs 32-byte elements); carry and index
   come back to the host.  For a prover that goes on to commit to the witness on the GPU, and the form bench.py times
   (--workload lhs_witness: inputs and outputs resident). */
int lemsm_lhs_witness_device(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine, size_t n,
                             uint8_t base, uint64_t out_carry[12], void* d_out_coeffs, size_t cap_coeffs, size_t* out_index,
                             int normalise, size_t* bad_index);
/* A rank's share of it: only the functions [f_begin, f_end) of the d of the call are computed (out_index rows of the
   others read length 0).  The d merge trees are independent, so a node shards compute_lhs_witness by digit position with
   no exchange (halo2_liam_eagen_msm_amd.dist.window_range gives the split); every rank runs the MSM core for the carries. */
int lemsm_lhs_witness_device_range(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine, size_t n,
                                   uint8_t base, uint32_t f_begin, uint32_t f_end, uint64_t out_carry[12], void* d_out_coeffs,
                                   size_t cap_coeffs, size_t* out_index, int normalise, size_t* bad_index);
/* Host-clock milliseconds of the four phases of the last lemsm_lhs_witness call (each ends on a stream synchronise):
   [0] the MSM core (upload of scalars and points, digits, buckets, carries), [1] the table of multiples and the d point
   lists, [2] the merge forest (every field operation of the divisor witnesses), [3] the download of the coefficients
   into the caller's buffer (32 B each over PCIe; pageable memory is paged in by this copy). */
int lemsm_lhs_witness_last_phases(const lemsm_ctx* ctx, double out_ms[4]);

/* ---- RegularFunction::ev: evaluating divisor witnesses -------------------------------- */
/* RegularFunction::ev / ev_unchecked (src/regular_functions_utils.rs:228-237; Polynomial::ev :41-43), the one thing the
   reference does with a witness (its tests :638-671, the argument's challenge points src/config.rs:224-283): for T functions
   a(x) + y b(x) and a batch of points, ev_unchecked(x, y) = a(x) + y b(x), exact in bn256::Fr; an empty polynomial is 0.
   Grumpkin only, like the divisor-witness entries.
   index: T x 4 entries {offset_a, len_a, offset_b, len_b} in 32-byte elements into the coefficient buffer (constant term
   first) -- the layout lemsm_lhs_witness* and lemsm_divisor_witness_batch write, rows of length (0, 0) included (they
   evaluate to 0).  points: K x 8 limbs affine, taken literally (no on-curve test; (0,0) gives a[0]), or, jacobian != 0,
   K x 12 limbs with x = X/Z^2, y = Y/Z^3 (:229-231); Z == 0 is the reference's invert().unwrap() panic (:230):
   LEMSM_ERR_DIVISION_BY_ZERO, the first such point's index in *bad_index, out_values untouched.
   counts == NULL: the K points are shared by all functions; value (t, k) is out_values[(t K + k) * 4 ..].
   counts != NULL: function t has its own counts[t] points, lists concatenated (as lemsm_divisor_witness_batch);
   K must be sum(counts) (LEMSM_ERR_LEN_MISMATCH); value k belongs to point k.
   out_values: num_values x 4 raw-Montgomery limbs.  T == 0, K == 0 and functions with no points are allowed. */
/* Pure host: validates a request and prices it.  num_values = T K (shared points) or K (lists); field_mults =
   sum_t (len_a + len_b) points_t, the Horner count; coeff_bytes = 32 sum (len_a + len_b) over functions with at least one
   point, what one pass over the coefficients reads.  LEMSM_ERR_BAD_ARG: a row with offset + len > cap_coeffs (or wrapping).
   (RegularFunction::ev, :228-237) */
int lemsm_regfn_eval_plan(const size_t* index, size_t T, size_t cap_coeffs, const size_t* counts, size_t K, size_t* num_values,
                          uint64_t* field_mults, uint64_t* coeff_bytes);
/* Coefficients resident in the context's HBM (d_coeffs: cap_coeffs 32-byte elements, e.g. what lemsm_lhs_witness_device
   left there); index, points, counts and out_values in host memory.  Every coefficient is read from HBM once per tile of
   four points.  (RegularFunction::ev / ev_unchecked, :228-237) */
int lemsm_regfn_eval_device(lemsm_ctx* ctx, int curve, const void* d_coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                            const uint64_t* points, int jacobian, const size_t* counts, size_t K, uint64_t* out_values,
                            size_t* bad_index);
/* The same with the coefficients in host memory (uploaded, then the device path).  (:228-237) */
int lemsm_regfn_eval(lemsm_ctx* ctx, int curve, const uint64_t* coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                     const uint64_t* points, int jacobian, const size_t* counts, size_t K, uint64_t* out_values,
                     size_t* bad_index);
/* Device time (ms, HIP events on the context's stream) of the evaluation launches of the last lemsm_regfn_eval* call --
   power tables, tile kernel, fold -- and the plan's coeff_bytes and field_mults: the figures its HBM and VALU rooflines
   are priced with (as lemsm_divisor_last_ntt).  (:228-237) */
int lemsm_regfn_eval_last(const lemsm_ctx* ctx, double* ms, uint64_t* coeff_bytes, uint64_t* field_mults);

/* ---- the left-hand side of the argument: L(f) of divisor witnesses -------------------- */
/* The identity the argument compares is
     sum_f (-base)^f L(f_f)  =  g(-R) + sum_j sum_k bucket[j][k] g(k P_j),   g(P) = (Ax - x_P) / (y_P - t x_P + t Ax - Ay).
   L(f), for f = a(x) + y b(x), is the derivative in the slope lambda, at the tangent slope t of the challenge point A, of
   log f(B(lambda)) + log f(C(lambda)), B and C the two other intersections of the curve with the line of slope lambda
   through A; at lambda = t they are A and -2A.  With (Cx, Cy) = -2A, dS = 2 t, dQ = 2 t Ax - 2 Ay and, for (Bx, By, Ox) in
   {(Ax, Ay, Cx), (Cx, Cy, Ax)}, dBx = (Bx dS - dQ) / (Bx - Ox), dBy = (Bx - Ax) + t dBx:
     L(f) = sum over the two of ((a'(Bx) + By b'(Bx)) dBx + b(Bx) dBy) / (a(Bx) + By b(Bx)).
   L is invariant under scaling f, so either `normalise` of lemsm_lhs_witness* gives the same bytes.
   Grumpkin only (LEMSM_ERR_BAD_CURVE otherwise, as the eval entries).  index / coefficients: as lemsm_regfn_eval*.  a_xy:
   K x 8 limbs, K challenge points, each an affine point of the curve (off the curve: LEMSM_ERR_BAD_ARG, Ay == 0:
   LEMSM_ERR_DIVISION_BY_ZERO, both with the challenge's index in *bad_index); t is always the tangent 3 Ax^2 / (2 Ay)
   (lemsm_slope) -- unlike the rhs entry, which takes any t, the formula for L holds only there -- and is returned in out_t.
   base: 3 .. 255 (LEMSM_ERR_BAD_BASE); function f, the row index, gets the weight (-base)^f: the order in which
   lemsm_lhs_witness* returns the functions.  A row with len_a = len_b = 0 is skipped: its L is 0 and it is absent from
   the sum -- the rows lemsm_lhs_witness_device_range leaves for the other ranks' functions, so each rank of a sharded
   witness gets the partial sum over its own functions and the host adds K field elements.
   f(A) == 0 or f(-2A) == 0 for a non-empty function (L has a pole): LEMSM_ERR_DIVISION_BY_ZERO, *bad_index = the lowest
   f K + k, outputs untouched.
   out_L: T x K x 4 limbs, L of function f at challenge k in row f K + k; out_sum: K x 4, sum_f (-base)^f L[f][k]; out_t: K x 4.
   Each may be NULL.  T == 0 and K == 0 are allowed (T == 0: sums are zero). */
/* Pure host: validates the rows exactly as lemsm_regfn_eval_plan and prices a call: num_values = T K; field_mults =
   4 K sum (len_a + len_b) (two abscissae, value and derivative each: the dual Horner's products); coeff_bytes =
   32 sum (len_a + len_b), what one pass over the coefficients reads (0 when K == 0: nothing is read). */
int lemsm_regfn_logderiv_plan(const size_t* index, size_t T, size_t cap_coeffs, size_t K, size_t* num_values, uint64_t* field_mults,
                              uint64_t* coeff_bytes);
/* Coefficients resident in the context's HBM (what lemsm_lhs_witness_device left there); everything else in host memory.
   Every coefficient is read from HBM once per challenge. */
int lemsm_regfn_logderiv_device(lemsm_ctx* ctx, int curve, const void* d_coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                                const uint64_t* a_xy, size_t K, uint8_t base, uint64_t* out_L, uint64_t* out_sum, uint64_t* out_t,
                                size_t* bad_index);
/* The same with the coefficients in host memory (uploaded, then the device path). */
int lemsm_regfn_logderiv(lemsm_ctx* ctx, int curve, const uint64_t* coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                         const uint64_t* a_xy, size_t K, uint8_t base, uint64_t* out_L, uint64_t* out_sum, uint64_t* out_t,
                         size_t* bad_index);
/* Device time (ms, HIP events around the launches) of the last lemsm_regfn_logderiv* call and its plan's figures. */
int lemsm_regfn_logderiv_last(const lemsm_ctx* ctx, double* ms, uint64_t* coeff_bytes, uint64_t* field_mults);
/* Test hook: the polynomial values the L kernels work from.  For T functions (coefficients in host memory) and K pairs of
   arbitrary field elements xs (2 K x 4 limbs; no curve involved, 0 allowed), out = T x K x 2 x 4 field elements
   {a(x), a'(x), b(x), b'(x)} for the two x of pair k, row ((f K + k) 2 + s) 4. */
int lemsm_debug_regfn_deriv(lemsm_ctx* ctx, const uint64_t* coeffs, size_t cap_coeffs, const size_t* index, size_t T, const uint64_t* xs,
                            size_t K, uint64_t* out);
/* Host only: out = lhs_sum - g(-R) + rhs_sum, zero exactly when the argument closes.  lhs_sum: out_sum of
   lemsm_regfn_logderiv*; rhs_sum: out_sum of lemsm_rhs_witness* (it already carries the gate's minus sign); R: the carry of
   lemsm_lhs_witness* as 12 Jacobian limbs, made affine here; a_xy, t: the challenge and its slope (out_t).  Field elements
   of the base field of `curve` (both curves).  R = O (Z == 0): g(O) := 0 -- the identity holds with that value (the sum of
   the digit lists' divisors then has no pole left to account for; tests/test_logderiv_plan.py checks it on inputs whose
   sum is the identity).  -R on the line through A: LEMSM_ERR_DIVISION_BY_ZERO. */
int lemsm_argument_residual(int curve, const uint64_t lhs_sum[4], const uint64_t carry_jacobian[12], const uint64_t rhs_sum[4],
                            const uint64_t a_xy[8], const uint64_t t[4], uint64_t out[4]);

/* ---- the right-hand side: bucket-weighted line sums ("rhs main" gate, src/config.rs:504-538) ---- */
/* The cells the reference's "rhs main" gate fixes down column c (src/config.rs:504-538; synthesize is a stub upstream,
   :635-683): for n scalars / points, base - 1 chains, one per non-zero digit value k, each stepping one scalar at a time
   (Rotation(-sc_box_size), :507):
     running[j][k-1] = init[k-1] + sum_{j' <= j} term(j', k),
     term(j, k) = - bucket[j][k] (Ax - x) / (y - t x + f),  f = t Ax - Ay  (:519-524),  (x, y) = k P_j (the fixed column of :542-560),
     bucket[j][k] = sum over the digit positions i < d with digit_{j,i} == k of (-base)^i, reduced into the field
   (Entry::Bucket of row k, src/negbase_utils.rs:97,115, taken from the digits themselves: no i128 overflow), digits =
   the negabase digits of scalar j, LSB first, d = lemsm_num_digits, padded as src/argument_witness_calc.rs:99.
   All field elements are raw Montgomery limbs of the BASE field of `curve`; term index = j (base - 1) + (k - 1).
   A term whose bucket is zero is zero whatever its denominator.  A zero denominator under a non-zero bucket (k P_j in
   {A, -2A}: the gate has no solution) is LEMSM_ERR_DIVISION_BY_ZERO with the first such term's index in *bad_index; a scalar
   >= isqrt(order) + 2 (:97) is LEMSM_ERR_SCALAR_OUT_OF_RANGE with its index in *bad_index.  On an error status nothing but
   *bad_index is defined.  A = (Ax, Ay) need not lie on the curve and t need not be its tangent slope (lemsm_slope,
   src/config.rs:184-187).  Both curves, base 3..255, n = 0 allowed (totals = init). */
/* Pure host: validates (curve, base >= 3: LEMSM_ERR_BAD_BASE) and prices a call: num_terms = n (base - 1); table_bytes = 64 num_terms;
   out_bytes = 32 num_terms; field_mults = the field multiplications of the shipped kernels per call: with T = num_terms,
   R = 256 ceil(T / 4096) (one root per thread of the batched inversion) and rk = min(32, max(1, R / 1024)) roots per inverting
   thread, 7 T + 3 R + 384 ceil(R / rk) -- per term 3 for the term itself (bucket into Montgomery form, t x, bucket (x - Ax)), 1 for
   the prefix product, 3 to apply the inverse; 3 per root; 384 for a Fermat inversion.  size_t overflow of 64 n (base - 1):
   LEMSM_ERR_BAD_ARG.  (src/config.rs:504-538) */
int lemsm_rhs_plan(int curve, uint8_t base, size_t n, size_t* num_terms, uint64_t* table_bytes, uint64_t* out_bytes, uint64_t* field_mults);
/* The fixed column of src/config.rs:542-560 left in HBM: d_out_table = n (base - 1) rows of 64 B, row j (base - 1) + (k - 1) =
   affine k P_j, bit-identical to what lemsm_precompute_multiplicities_affine returns for the same points (d_points_affine:
   n x 64 B affine rows, read as Jacobian with Z = 1; an all-zero row is the identity). */
int lemsm_multiples_table_device(lemsm_ctx* ctx, int curve, const void* d_points_affine, size_t n, uint8_t base, void* d_out_table);
/* Scalars (n x 32 B) and table (as above; rows are taken literally, no on-curve test) resident in HBM; d_out_running
   (n (base - 1) x 32 B, row-major [j][k-1]) stays in HBM and may be NULL: totals only, no cell is written.  a_xy: 8 limbs, t: 4 limbs,
   init: (base - 1) x 4 limbs or NULL = zeros.  out_totals ((base - 1) x 4, optional) = running[n-1][.]; out_sum (optional) = their
   sum, the double sum of the argument's right-hand side with the gate's sign.  (src/config.rs:504-538) */
int lemsm_rhs_witness_device(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_table, size_t n, uint8_t base,
                             const uint64_t a_xy[8], const uint64_t t[4], const uint64_t* init, void* d_out_running,
                             uint64_t* out_totals, uint64_t out_sum[4], size_t* bad_index);
/* Host pointers, the points as the reference holds them (n x 12 limbs Jacobian, any Z; src/argument_witness_calc.rs:43-51):
   builds the table on the device, runs the device path, downloads the running sums when out_running != NULL.
   (src/config.rs:504-538, :542-560) */
int lemsm_rhs_witness(lemsm_ctx* ctx, int curve, const uint8_t* scalars, const uint64_t* pts_jacobian, size_t n, uint8_t base,
                      const uint64_t a_xy[8], const uint64_t t[4], const uint64_t* init, uint64_t* out_running,
                      uint64_t* out_totals, uint64_t out_sum[4], size_t* bad_index);
/* The engine on its own, for the log-derivative lookup columns (src/config.rs:402-437: c[i+1] - c[i] = 1 / (v - b[i+1])):
   out[i] = (i < chains ? init[i] : out[i - chains]) + num[i] / den[i] over n field elements of the BASE field of `curve`.
   d_num == NULL means every numerator is 1.  num = 0 gives 0 whatever den; den = 0 otherwise: LEMSM_ERR_DIVISION_BY_ZERO with the
   first such index in *bad_index.  chains >= 1 (0: LEMSM_ERR_BAD_ARG), n arbitrary (also n < chains); init: chains x 4 limbs or
   NULL = zeros; d_out_running (n x 32 B) may be NULL; out_totals: chains x 4, the last cell of each chain (init where a
   chain is empty). */
int lemsm_fraction_sums_device(lemsm_ctx* ctx, int curve, const void* d_num, const void* d_den, size_t n, size_t chains,
                               const uint64_t* init, void* d_out_running, uint64_t* out_totals, size_t* bad_index);
/* The same with num (may be NULL), den and out_running (may be NULL) in host memory.  (src/config.rs:402-437) */
int lemsm_fraction_sums(lemsm_ctx* ctx, int curve, const uint64_t* num, const uint64_t* den, size_t n, size_t chains,
                        const uint64_t* init, uint64_t* out_running, uint64_t* out_totals, size_t* bad_index);
/* Device time (ms, HIP events around the launches on the context's stream) of the last lemsm_rhs_witness* /
   lemsm_fraction_sums* call and the bytes / field_mults its plan prices it with (rhs: table_bytes, plus out_bytes when
   the running sums were written; fractions: 32 B per element read and written, 4 n + 3 R + 384 ceil(R / rk) products).
   (src/config.rs:504-538, :402-437) */
int lemsm_rhs_last(const lemsm_ctx* ctx, double* ms, uint64_t* bytes, uint64_t* field_mults);

/* ---- advice column a and its polynomial-RLC cells (src/layout.md:7, src/config.rs:246-283) ---- */
/* In the reference's circuit the coefficients of the d divisor witnesses ARE advice column a: one batch of batch_size rows
   holds the same coefficient of each function (src/layout.md:7, src/layout.md.bac:30-34), batch_size = T + batch_offset
   (params_check, src/config.rs:45) with T the number of index rows -- the functions lemsm_lhs_witness* actually returns, not
   params_check's num_digits (:42), which is one short of compute_lhs_witness's d and overflows its u8 for base >= 16.
   Row f < T of a batch belongs to function f (index row f); rows T .. batch_size - 1 are zero.  "The same coefficient" is the
   same monomial, the monomials in pole order (x^i: 2 i, y x^i: 2 i + 3, as `normalise` orders them; order 1 does not exist):
     batch 0 = a_0,  batch 2 i - 1 = a_i (i >= 1),  batch 2 i + 2 = b_i;   row j batch_size + f = monomial j of function f.
   A function needs max(row(a_{len_a - 1}), row(b_{len_b - 1})) + 1 batches (0 when empty); batches with no coefficient of a
   function hold zero in its row; num_batches = the largest such count, or a larger caller-given value (upstream pads to
   N + B + 1, src/layout.md.bac:19): the surplus batches are zero.
   The "polynomials random linear combination" gate (src/config.rs:246-283; synthesize is a stub, :635-683) fixes the last
   c_skip = ceil(batch_size / poly_fan_in) rows (:46) of each batch in column c: with F = poly_fan_in, for t < c_skip
     c_0 = sum_i r^i a[j][i c_skip],   c_t = c_{t-1} r^F + sum_i r^i a[j][t + i c_skip]   (t >= 1),
   term i < F present exactly when t + i c_skip < batch_size (the gate's full form where its last operand is a row of the
   batch, its truncated form :273-276 where it is not; the selectors as written, :299-325, never enable the full form and can
   reach into the next batch -- DESIGN 7b).  Every row of the batch enters exactly once: the last cell is
   sum_i r^e(i) a[j][i], e(i) = floor(i / c_skip) + F (c_skip - 1 - i mod c_skip).
   Grumpkin only (LEMSM_ERR_BAD_CURVE otherwise), like the witness entries: the cells lie in bn256::Fr. */
enum lemsm_form {
  LEMSM_FORM_MONTGOMERY = 0,   /* 4 raw Montgomery limbs: the cells as halo2 holds advice values, what every field kernel reads */
  LEMSM_FORM_CANONICAL = 1     /* 32-byte little-endian standard form: what the MSM entries take as scalars */
};
/* Pure host: validates a layout and prices it.  index: T x 4 rows as lemsm_regfn_eval_plan validates them (offset + len
   past cap_coeffs or wrapping: LEMSM_ERR_BAD_ARG); poly_fan_in == 0, num_batches != 0 but smaller than the functions need,
   or a row count whose bytes overflow size_t: LEMSM_ERR_BAD_ARG.  num_batches == 0: the minimum.  T == 0 is allowed.
   rows = num_batches batch_size, cells = num_batches c_skip.  The floor's ingredients: the assembly reads coeff_bytes =
   32 sum (len_a + len_b) and writes column_bytes = 32 rows, with assembly_field_mults = sum (len_a + len_b) products for
   the canonical form (none for the Montgomery form); the RLC reads column_bytes, writes 32 cells and takes
   rlc_field_mults products: per batch one per row plus the scan's (per 64 cells sum over off = 1, 2, 4 .. < n of n - off,
   n the cells of that group, and n more for every group after the first).  (src/config.rs:39-48, :246-283) */
int lemsm_column_plan(const size_t* index, size_t T, size_t cap_coeffs, size_t batch_offset, size_t poly_fan_in, size_t num_batches,
                      size_t* out_batch_size, size_t* out_c_skip, size_t* out_num_batches, size_t* out_rows, size_t* out_cells,
                      uint64_t* coeff_bytes, uint64_t* column_bytes, uint64_t* assembly_field_mults, uint64_t* rlc_field_mults);
/* Column a from coefficients resident in HBM (d_coeffs, cap_coeffs, index, T: as lemsm_regfn_eval_device takes them, e.g.
   what lemsm_lhs_witness_device left there) into d_out_column: rows x 32 B in HBM, in `form`.  The canonical form is exactly
   what lemsm_msm_device(LEMSM_BN254_G1, ...) takes as scalars: bn256::Fr is the scalar field of BN254 G1, so the first-phase
   commitment to the column is that MSM.  num_batches: 0 = minimal; *out_num_batches (optional) = the count laid out.
   cap_rows < rows: LEMSM_ERR_BAD_ARG, the output is untouched and no work is left queued (as the witness entries).
   (src/layout.md:7, src/layout.md.bac:30-34) */
int lemsm_column_a_device(lemsm_ctx* ctx, int curve, const void* d_coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                          size_t batch_offset, size_t num_batches, int form, void* d_out_column, size_t cap_rows, size_t* out_num_batches);
/* The same with the coefficients and the column in host memory (uploaded, the device path, downloaded).  (src/layout.md:7) */
int lemsm_column_a(lemsm_ctx* ctx, int curve, const uint64_t* coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                   size_t batch_offset, size_t num_batches, int form, uint64_t* out_column, size_t cap_rows, size_t* out_num_batches);
/* The gate's cells from a column a resident in HBM (d_column: num_batches (T + batch_offset) x 32 B in `form`; a canonical
   column costs nothing extra, the factor is folded into the power table).  r: the challenge, 4 raw Montgomery limbs
   (not canonical: LEMSM_ERR_BAD_ARG).  d_out_cells: num_batches c_skip x 32 B, raw Montgomery like every other cell entry,
   cell (j, t) at j c_skip + t.  Sums run in a fixed order: repeated calls, and the host and the device entry, give the same
   bytes.  cap_cells too small: LEMSM_ERR_BAD_ARG, output untouched.  (src/config.rs:246-283) */
int lemsm_poly_rlc_device(lemsm_ctx* ctx, int curve, const void* d_column, int form, size_t T, size_t batch_offset, size_t poly_fan_in,
                          size_t num_batches, const uint64_t r[4], void* d_out_cells, size_t cap_cells);
/* The same with the column and the cells in host memory.  (src/config.rs:246-283) */
int lemsm_poly_rlc(lemsm_ctx* ctx, int curve, const uint64_t* column, int form, size_t T, size_t batch_offset, size_t poly_fan_in,
                   size_t num_batches, const uint64_t r[4], uint64_t* out_cells, size_t cap_cells);
/* Device time (ms, HIP events around the launch on the context's stream) of the last lemsm_column_a* / lemsm_poly_rlc* call,
   and the bytes (read + written) and field multiplications its plan prices it with.  (src/config.rs:246-283) */
int lemsm_column_last(const lemsm_ctx* ctx, double* ms, uint64_t* bytes, uint64_t* field_mults);

/* ---- halo2::arithmetic on resident data: best_fft, kate_division, the Polynomial product -------------------------------
   (src/regular_functions_utils.rs:5 imports best_fft, best_multiexp, eval_polynomial, kate_division) --------- */
/* Everything here is over bn256::Fr (Grumpkin's base field, the scalar field of BN254 G1, the one FftPrecomp field:
   src/precomputed_fft_data.rs:3); an element is 32 bytes, 4 raw Montgomery limbs, as for every other cell entry.  The
   entries keep the conventions of the witness entries: a capacity that is too small is LEMSM_ERR_BAD_ARG with the lengths
   set, the output untouched and nothing left queued; a field argument that is not canonical is LEMSM_ERR_BAD_ARG; sums run
   in a fixed order, so the host entry, the device entry and repeated calls give the same bytes; option ws_canary guards
   every carved workspace.
   eval_polynomial (:42, Polynomial::ev) has no entry of its own: lemsm_regfn_eval_device with index rows
   {offset, len, 0, 0} (an empty b part) and affine points (x, anything) is Polynomial::ev at x. */
/* The FftPrecomp trait (:17-24), pure host.  omega: omega_pow(28 - logn), or omega_pow_inv(28 - logn) with inverse != 0:
   the generator of the 2^logn-th roots of unity the reference uses (logn 0 .. 28; more: LEMSM_ERR_BAD_ARG). */
int lemsm_fft_omega(uint32_t logn, int inverse, uint64_t out[4]);
/* half_pow(exp) = 2^-exp (:22; exp < 64, the length of the reference's table; more: LEMSM_ERR_BAD_ARG) */
int lemsm_fft_half_pow(uint64_t exp, uint64_t out[4]);
/* Pure host: prices nseq transforms of 2^logn elements.  logn 0 .. 26, nseq >= 1, nseq << logn <= 2^28 (else
   LEMSM_ERR_BAD_ARG).  passes = the LDS-tiled passes over HBM (one of up to 10 stages, then one per 8 stages more) plus one
   for the reordering; bytes = 64 (nseq << logn) passes; butterflies = nseq logn 2^(logn-1), one field product each.
   (halo2 best_fft, called at :119-124) */
int lemsm_fft_plan(uint32_t logn, size_t nseq, uint32_t* passes, uint64_t* bytes, uint64_t* butterflies);
/* halo2's best_fft(a, omega, log_n) (:119-124), in place on nseq sequences of 2^logn elements resident at d_data, natural
   order in and out: a[k] <- scale sum_j a[j] omega^(j k).  scale == NULL: unscaled, as best_fft leaves it; otherwise the
   factor is folded into the reordering pass (mul_fft's half_pow, an inverse transform's 1/n).  omega must be a primitive
   2^logn-th root of unity (omega^(2^(logn-1)) == -1; omega == 1 for logn 0), else LEMSM_ERR_BAD_ARG: an inverse transform
   is the same call with omega^-1.  The table omega^t, t < 2^(logn-1) (32 B 2^(logn-1): 1 GB at 2^26) is kept in the
   context for the next call with the same (omega, logn); no memory for it: LEMSM_ERR_NOMEM. */
int lemsm_fft_device(lemsm_ctx* ctx, void* d_data, size_t nseq, uint32_t logn, const uint64_t omega[4], const uint64_t* scale);
/* The same with host arrays (uploaded, the device path, downloaded); in == out is allowed.  (best_fft, :119-124) */
int lemsm_fft(lemsm_ctx* ctx, const uint64_t* in, uint64_t* out, size_t nseq, uint32_t logn, const uint64_t omega[4], const uint64_t* scale);
/* Polynomial::kate_div (:45-47), halo2's kate_division(a, b): the quotient of a(x) by (x - b), remainder dropped, of T rows
   that share b (the two parts of a RegularFunction in merge, :357).  index: T x 2 rows {offset, len} in elements of d_in;
   the quotient of row t lies at the same offset of d_out and has len - 1 coefficients: q[len-2] = a[len-1],
   q[i] = a[i+1] + b q[i+1].  A row of length 1 gives an empty row.  A row of length 0 is the reference's vec![0; len - 1]
   underflow: LEMSM_ERR_ARITH_OVERFLOW, the row in *bad_index (optional), nothing written.  A row reaching past cap_in, a
   quotient reaching past cap_out, two rows that overlap, or d_out overlapping d_in (the byte ranges of the two
   capacities): LEMSM_ERR_BAD_ARG, nothing written. */
int lemsm_kate_division_device(lemsm_ctx* ctx, const void* d_in, size_t cap_in, const size_t* index, size_t T, const uint64_t b[4],
                               void* d_out, size_t cap_out, size_t* bad_index);
/* The same with host arrays; only the quotient rows of `out` are written.  (:45-47) */
int lemsm_kate_division(lemsm_ctx* ctx, const uint64_t* in, size_t cap_in, const size_t* index, size_t T, const uint64_t b[4],
                        uint64_t* out, size_t cap_out, size_t* bad_index);
/* &p * &q (impl Mul, :209-216) of la and lb coefficients resident in HBM: *len_out = la + lb - 1 coefficients at d_out.
   la == lb == 0 is the usize underflow of :55: LEMSM_ERR_ARITH_OVERFLOW.  Exactly one empty operand: la + lb - 1 zeros,
   what mul_naive returns.  la + lb - 1 > 2^26, or cap_out too small (then *len_out is set and the output untouched), or
   the product's bytes overlapping an operand: LEMSM_ERR_BAD_ARG.  The arithmetic is exact, so which of the reference's two
   algorithms ran does not show in the bits: an operand of fewer than 32 coefficients takes the direct kernel (mul_naive,
   :54-62), anything else two forward transforms, one pointwise pass and one inverse transform (mul_fft, :102-129). */
int lemsm_poly_mul_device(lemsm_ctx* ctx, const void* d_a, size_t la, const void* d_b, size_t lb, void* d_out, size_t cap_out, size_t* len_out);
/* The same with host arrays.  (:209-216) */
int lemsm_poly_mul(lemsm_ctx* ctx, const uint64_t* a, size_t la, const uint64_t* b, size_t lb, uint64_t* out, size_t cap_out, size_t* len_out);
/* Device time (ms, HIP events around the launches on the context's stream) of the last lemsm_fft* / lemsm_kate_division* /
   lemsm_poly_mul* call, and the bytes and field multiplications it is priced at.  (:45-47, :102-129, :209-216) */
int lemsm_poly_last(const lemsm_ctx* ctx, double* ms, uint64_t* bytes, uint64_t* field_mults);

/* ---- Multipoint openings on resident polynomials: combine, divide by roots --------------------------------
   The polynomial work of the last round of a halo2 proof (GWC or SHPLONK): q = (sum_j c_j p_j - r) / prod_i (X - z_i) over
   polynomials that stay in HBM.  bn256::Fr, 32-byte raw Montgomery elements, the conventions of the entries above: a field
   argument that is not canonical is LEMSM_ERR_BAD_ARG, LEMSM_ERR_BAD_ARG leaves nothing queued and the outputs untouched
   (a capacity that is too small sets the length output first), the figures of every call go to lemsm_poly_last, option
   ws_canary guards every carved workspace.  The arithmetic is exact and every sum runs in one fixed order: the host entry,
   the device entry and a repeated call give the same bytes. */
#define LEMSM_OPEN_MAX_ROOTS 8       /* roots of one division, coefficients of `low` */
#define LEMSM_OPEN_MAX_POLYS 4096    /* polynomials of one combination */
/* out[i] = sum_{j : i < lens[j]} c_j p_j[i] - (i < k_low ? low[i] : 0) for i < *len_out = max(max_j lens[j], k_low).
   d_polys: J device pointers, polynomial j has lens[j] coefficients (ragged, any length up to 2^28; lens[j] == 0 is allowed
   and its pointer may be NULL); coeffs: J x 4 limbs c_j; low: k_low <= LEMSM_OPEN_MAX_ROOTS host coefficients (the r(X) of a
   rotation set, the single evaluation of GWC), NULL means k_low = 0.  J == 0, J > LEMSM_OPEN_MAX_POLYS, a length above
   2^28, cap_out < *len_out (in coefficients), or the output's *len_out coefficients overlapping an operand:
   LEMSM_ERR_BAD_ARG.  lemsm_poly_last: bytes = 32 (sum_j lens[j] + *len_out), field_mults = sum_j lens[j]. */
int lemsm_poly_lincomb_device(lemsm_ctx* ctx, const void* const* d_polys, const size_t* lens, size_t J, const uint64_t* coeffs,
                              const uint64_t* low, size_t k_low, void* d_out, size_t cap_out, size_t* len_out);
/* The same with host arrays (uploaded, the device path, downloaded). */
int lemsm_poly_lincomb(lemsm_ctx* ctx, const uint64_t* const* polys, const size_t* lens, size_t J, const uint64_t* coeffs,
                       const uint64_t* low, size_t k_low, uint64_t* out, size_t cap_out, size_t* len_out);
/* a_0 = the len coefficients at d_in, a_(i+1) = kate_division(a_i, z_i) for the k roots z_i (k x 4 limbs, 1 <= k <=
   LEMSM_OPEN_MAX_ROOTS; repeated roots and 0 are legal): a_k, len - k coefficients, goes to d_out in `form`
   (LEMSM_FORM_MONTGOMERY, or LEMSM_FORM_CANONICAL: the scalars lemsm_msm_device takes).  out_rem (host, k x 4 limbs,
   Montgomery, optional): out_rem[i] = a_i(z_i), the remainder stage i drops; all zero exactly when prod (X - z_i) divides a.
   The intermediate quotients live in the call's workspace; only a_k touches d_out.  len == k gives an empty quotient.
   len < k hands stage `len` an empty polynomial, the reference's len - 1 underflow: LEMSM_ERR_ARITH_OVERFLOW, the stage
   in *bad_index (optional) and lemsm_last_bad_index, nothing written.  k == 0, k > LEMSM_OPEN_MAX_ROOTS, len > 2^28, an
   unknown form, cap_out < len - k, or d_out overlapping d_in: LEMSM_ERR_BAD_ARG.  lemsm_poly_last: 96 B and 2 products per
   coefficient of every a_i, i < k (as lemsm_kate_division_device prices a row), and 64 B and 1 product per coefficient of
   a_k for the canonical form. */
int lemsm_poly_divide_roots_device(lemsm_ctx* ctx, const void* d_in, size_t len, const uint64_t* roots, size_t k, int form,
                                   void* d_out, size_t cap_out, uint64_t* out_rem, size_t* bad_index);
/* The same with host arrays. */
int lemsm_poly_divide_roots(lemsm_ctx* ctx, const uint64_t* in, size_t len, const uint64_t* roots, size_t k, int form,
                            uint64_t* out, size_t cap_out, uint64_t* out_rem, size_t* bad_index);
/* q = (sum_j c_j p_j - low) / prod_i (X - z_i) in one call: the combination of lemsm_poly_lincomb_device into the call's
   workspace, then the stages of lemsm_poly_divide_roots_device into d_out; *len_out = max(max_j lens[j], k_low) - k.  The
   statuses and figures of both (the capacity and the overlap are those of the quotient). */
int lemsm_open_quotient_device(lemsm_ctx* ctx, const void* const* d_polys, const size_t* lens, size_t J, const uint64_t* coeffs,
                               const uint64_t* low, size_t k_low, const uint64_t* roots, size_t k, int form,
                               void* d_out, size_t cap_out, size_t* len_out, uint64_t* out_rem, size_t* bad_index);
/* The same with host arrays. */
int lemsm_open_quotient(lemsm_ctx* ctx, const uint64_t* const* polys, const size_t* lens, size_t J, const uint64_t* coeffs,
                        const uint64_t* low, size_t k_low, const uint64_t* roots, size_t k, int form,
                        uint64_t* out, size_t cap_out, size_t* len_out, uint64_t* out_rem, size_t* bad_index);
/* Pure host: what lemsm_open_quotient_device does for these lengths (k == 0: the combination alone, as
   lemsm_poly_lincomb_device).  len = max(max_j lens[j], k_low); *len_out = len - k; *bytes = 32 (sum_j lens[j] + len) +
   sum_{i<k} 96 (len - i); *field_mults = sum_j lens[j] + sum_{i<k} 2 (len - i) (Montgomery form); *workspace_bytes = the
   device workspace the call reserves (without guards).  Every output is optional.  len < k: LEMSM_ERR_ARITH_OVERFLOW. */
int lemsm_open_plan(const size_t* lens, size_t J, size_t k_low, size_t k, size_t* len_out, uint64_t* bytes, uint64_t* field_mults,
                    size_t* workspace_bytes);
/* Pure host: the k coefficients (k x 4 limbs, lowest first) of the polynomial of degree < k through (points[i], evals[i]),
   1 <= k <= LEMSM_OPEN_MAX_ROOTS: the r(X) of a rotation set.  Two equal points: LEMSM_ERR_DIVISION_BY_ZERO, the later
   index in *bad_index (optional), out_coeffs untouched. */
int lemsm_lagrange_interpolate(const uint64_t* points, const uint64_t* evals, size_t k, uint64_t* out_coeffs, size_t* bad_index);

/* ---- halo2's EvaluationDomain on resident data: coset and extended-domain transforms ---------------------
   bn256::Fr, 32-byte raw Montgomery elements, the conventions of the entries above (LEMSM_ERR_BAD_ARG leaves nothing
   queued and the outputs untouched; the figures of every call go to lemsm_poly_last).
   n = 2^logn, m = 2^logm, N = m n; w_ext = lemsm_fft_omega(logn + logm), w = w_ext^m = lemsm_fft_omega(logn),
   theta = w_ext^n; shift = g, any non-zero field element (halo2 passes F::ZETA); s_c = g w_ext^c generates coset c < m
   and t_c = s_c^n - 1 = g^n theta^c - 1 is the value of X^n - 1 on it.  The point with halo2's index e = c + m r is
   s_c w^r; `layout` says where its value lies.  Limits: logn <= 26, logm <= 4, logn + logm <= 28 (the 2-adicity of the
   field).  The mapping to halo2_proofs' poly/domain.rs is stated from memory; the formulas here are the contract. */
enum {
  LEMSM_EXT_INTERLEAVED = 0,   /* at element c + m r: halo2's ExtendedLagrangeCoeff order */
  LEMSM_EXT_COSET_MAJOR = 1    /* at element c n + r: a rotation is an index shift inside one coset */
};
/* Pure host: the price of one lemsm_coeff_to_extended_device call in the coset-major layout: passes over HBM (the spread,
   the tiled transform passes, the reorder), their bytes, the field products (butterflies, powers, the fold of
   coefficients past n) and the workspace bytes the call reserves.  The interleaved layout (logm > 0) and
   lemsm_extended_to_coeff_device reserve 32 N bytes more (the m sequences cannot stand in the caller's buffer); the
   latter runs the same passes plus the combine.  A limit exceeded or n_coeffs > N: LEMSM_ERR_BAD_ARG. */
int lemsm_domain_plan(uint32_t logn, uint32_t logm, size_t n_coeffs, uint32_t* passes, uint64_t* bytes, uint64_t* field_mults,
                      uint64_t* workspace_bytes);
/* Pure host, no context: out_t[c] = t_c, c < m, raw Montgomery limbs, zeros included (t_c == 0: coset c is the domain
   itself and lemsm_extended_to_coeff* cannot divide there).  shift zero or not canonical: LEMSM_ERR_BAD_ARG. */
int lemsm_vanishing_on_cosets(uint32_t logn, uint32_t logm, const uint64_t shift[4], uint64_t* out_t);
/* a[k] <- scale sum_j a[j] shift^j omega^(j k): the values on the coset shift <omega>, in place on nseq sequences, natural
   order in and out; omega and scale as lemsm_fft_device, nseq << logn <= 2^28.  shift == 1 gives the bytes of
   lemsm_fft_device.  The powers cost one more pass over the data (at most 3 products an element). */
int lemsm_coset_fft_device(lemsm_ctx* ctx, void* d_data, size_t nseq, uint32_t logn, const uint64_t omega[4], const uint64_t shift[4],
                           const uint64_t* scale);
/* a[j] <- scale shift_inv^j sum_k a[k] omega_inv^(j k): the inverse of the above with omega^-1, shift^-1 and scale = 1/n
   (lemsm_fft_half_pow(logn)); the powers ride on the reordering pass. */
int lemsm_coset_ifft_device(lemsm_ctx* ctx, void* d_data, size_t nseq, uint32_t logn, const uint64_t omega_inv[4], const uint64_t shift_inv[4],
                            const uint64_t* scale);
/* The same with host arrays (uploaded, the device path, downloaded); in == out is allowed. */
int lemsm_coset_fft(lemsm_ctx* ctx, const uint64_t* in, uint64_t* out, size_t nseq, uint32_t logn, const uint64_t omega[4], const uint64_t shift[4],
                    const uint64_t* scale);
int lemsm_coset_ifft(lemsm_ctx* ctx, const uint64_t* in, uint64_t* out, size_t nseq, uint32_t logn, const uint64_t omega_inv[4],
                     const uint64_t shift_inv[4], const uint64_t* scale);
/* EvaluationDomain::coeff_to_extended over a caller-chosen coset generator: P = sum_{j < n_coeffs} a[j] X^j, n_coeffs <= N
   (halo2 calls it with n; 0 gives zeros); writes P(s_c w^r) for all c < m, r < n to d_out (cap_out >= N elements, no
   overlap with d_coeffs) in `layout`.  m transforms of n elements over the size-n table, so N may be 2^28 where one
   transform stops at 2^26.  logm = 0 with shift = 1 is the plain transform. */
int lemsm_coeff_to_extended_device(lemsm_ctx* ctx, const void* d_coeffs, size_t n_coeffs, uint32_t logn, uint32_t logm, const uint64_t shift[4],
                                   int layout, void* d_out, size_t cap_out);
/* EvaluationDomain::extended_to_coeff, the exact inverse of the above for every polynomial of degree < N: from the N values
   at d_evals (in `layout`; with divide_vanishing != 0 each first divided by t_c: divide_by_vanishing_poly) the first
   n_out <= N coefficients to d_out (no overlap with d_evals) in `form`: LEMSM_FORM_MONTGOMERY, or LEMSM_FORM_CANONICAL, the
   scalars lemsm_msm_device takes.  Coefficients from n_out on are not written and not checked (halo2's truncation to
   n quotient_poly_degree).  divide_vanishing with some t_c == 0 (g = 1, for example): LEMSM_ERR_DIVISION_BY_ZERO with c in
   *bad_index (optional) and lemsm_last_bad_index, nothing written. */
int lemsm_extended_to_coeff_device(lemsm_ctx* ctx, const void* d_evals, uint32_t logn, uint32_t logm, const uint64_t shift[4], int layout,
                                   int divide_vanishing, int form, void* d_out, size_t n_out, size_t* bad_index);
/* The same two with host arrays. */
int lemsm_coeff_to_extended(lemsm_ctx* ctx, const uint64_t* coeffs, size_t n_coeffs, uint32_t logn, uint32_t logm, const uint64_t shift[4],
                            int layout, uint64_t* out, size_t cap_out);
int lemsm_extended_to_coeff(lemsm_ctx* ctx, const uint64_t* evals, uint32_t logn, uint32_t logm, const uint64_t shift[4], int layout,
                            int divide_vanishing, int form, uint64_t* out, size_t n_out, size_t* bad_index);

/* ---- gate expressions on the extended domain: the numerator of the quotient h (src/config.rs:232-568) ------
   What halo2's evaluate_h does over the custom gates of a circuit, on columns resident in HBM: every gate polynomial is
   evaluated at every point of the extended domain and the gates are combined by powers of the challenge y,
   h = (..(g_0 y + g_1) y + ..) y + g_last.  The circuit is data: a postfix program over the cells of the columns, the
   constants of the call (challenges among them) and the point itself.  The reference's gates (create_gate at
   src/config.rs:232, :246, :332, :402, :504, :562) are degree 4 over some twenty queried cells.
   Columns: one buffer of N = m n raw Montgomery elements each, in LEMSM_EXT_COSET_MAJOR -- the only layout these entries
   take: point (c, r) = s_c w^r (the definitions above) lies at element c n + r, and a query with rotation i reads row
   (r + i) mod n of the same coset, i.e. the column's polynomial at w^i X.  bn256::Fr, the conventions of the entries
   above.  The placement of rows and blinding stay with the caller.  LEMSM_GATE_PUSH_X and fixed columns make the terms of
   halo2's permutation and lookup arguments expressible; their grand product columns are built by
   lemsm_permutation_product* and lemsm_fraction_products* below. */
enum {  /* low 8 bits of a code word; operand = word >> 8 (zero for the opcodes that take none) */
  LEMSM_GATE_PUSH_CELL = 0,    /* q: push columns[queries[q].column] at row (r + queries[q].rotation) mod n of coset c */
  LEMSM_GATE_PUSH_CONST = 1,   /* k: push consts[k] (challenges are constants of a call) */
  LEMSM_GATE_PUSH_X = 2,       /* push the point itself, s_c w^r (permutation-style terms) */
  LEMSM_GATE_ADD = 3,          /* pop top, pop second, push second + top */
  LEMSM_GATE_SUB = 4,          /* ... second - top */
  LEMSM_GATE_MUL = 5,          /* ... second top */
  LEMSM_GATE_NEG = 6,          /* top <- -top */
  LEMSM_GATE_ADD_CELL = 7,     /* q: top <- top + cell q */
  LEMSM_GATE_SUB_CELL = 8,     /* q: top <- top - cell q */
  LEMSM_GATE_MUL_CELL = 9,     /* q: top <- top cell q */
  LEMSM_GATE_ADD_CONST = 10,   /* k: top <- top + consts[k] */
  LEMSM_GATE_SUB_CONST = 11,   /* k: top <- top - consts[k] */
  LEMSM_GATE_MUL_CONST = 12,   /* k: top <- top consts[k] */
  LEMSM_GATE_FOLD = 13         /* h <- h y + pop: halo2's combination of gates by powers of y; h starts at 0 */
};
typedef struct { int32_t column, rotation; } lemsm_gate_query;
typedef struct {
  const uint32_t* code; size_t n_code;
  const lemsm_gate_query* queries; size_t n_queries;
  const uint64_t* consts;      /* n_consts x 4 raw Montgomery limbs, canonical */
  size_t n_consts;
} lemsm_gate_program;
/* Pure host, no context: the validator (the device entry calls it too) and the price of a program per point.
   Limits: n_code <= 4096, n_queries, n_consts <= 256, ncols <= 64, stack depth <= 8, |rotation| < 2^26 (any rotation: it is
   reduced mod n).  A limit exceeded or a null pointer: LEMSM_ERR_BAD_ARG, *bad_index untouched.  Otherwise
   LEMSM_ERR_BAD_ARG with *bad_index (optional) set: a constant that is not canonical (the constant's index; every constant is
   checked, before any instruction); then, per instruction in the order unknown opcode, operand out of range (a query or
   constant index past its table, a query naming a column < 0 or >= ncols or a rotation past the limit, a non-zero operand
   field on an opcode that takes none), stack underflow, depth above 8 (the instruction's index); a stack that is not empty
   at the end, or a program without a FOLD (n_code).  A query that no instruction names is not looked at.
   stack_depth: the largest number of entries; folds: the FOLD count.  degree: in units of (n - 1), columns holding
   polynomials of degree < n: a cell or X counts 1, a constant 0, ADD / SUB take the maximum, MUL the sum; the maximum
   over the folds.  The extended domain must hold it: 2^logm >= degree (halo2's quotient drops one more unit).
   field_mults_per_point = #(MUL, MUL_CELL, MUL_CONST) + (folds - 1) + (3 if the program has a PUSH_X, however many): the
   first FOLD is h <- top, and the point is computed once per thread as one product by s_c and logn > 8 ? (logn > 16 ? 2 :
   1) : 0 for w^r; the plan does not know logn and prices the largest, lemsm_poly_last reports the call's own count.
   cell_loads_per_point = #(PUSH_CELL, ADD_CELL, SUB_CELL, MUL_CELL).  (halo2 evaluate_h; src/config.rs:232-568) */
int lemsm_gate_plan(const lemsm_gate_program* prog, size_t ncols, uint32_t* stack_depth, uint32_t* folds, uint32_t* degree,
                    uint64_t* field_mults_per_point, uint64_t* cell_loads_per_point, size_t* bad_index);
/* h on cosets coset_begin .. coset_begin + coset_count - 1: elements coset_begin n .. (coset_begin + coset_count) n - 1 of
   d_out (cap_out >= N elements, raw Montgomery) and nothing else, so a caller may work coset by coset or split the cosets
   over contexts.  d_columns: ncols device pointers, N elements each, coset-major.  shift = g as lemsm_coeff_to_extended_device
   took it: read only when the program has a PUSH_X (then NULL, zero or not canonical: LEMSM_ERR_BAD_ARG).  y: canonical.
   d_out must not overlap any column (rotations make an in-place run a race): LEMSM_ERR_BAD_ARG, as are a null pointer,
   coset_begin + coset_count > m, a limit exceeded (logn, logm as above), cap_out < N and a program lemsm_gate_plan refuses
   (*bad_index and lemsm_last_bad_index as there).  coset_count == 0 is LEMSM_OK and writes nothing.  One kernel, a thread
   per point, sums in program order: the same bytes on every call.  lemsm_poly_last: ms, bytes = (cell_loads_per_point + 1)
   32 points, and the products.  With lemsm_coeff_to_extended_device before and lemsm_extended_to_coeff_device(..,
   divide_vanishing = 1, ..) behind it this is halo2's vanishing argument without a download.
   (src/config.rs:232, :246, :332, :402, :504, :562) */
int lemsm_gate_eval_device(lemsm_ctx* ctx, const lemsm_gate_program* prog, const void* const* d_columns, size_t ncols, uint32_t logn,
                           uint32_t logm, uint32_t coset_begin, uint32_t coset_count, const uint64_t* shift, const uint64_t y[4], void* d_out,
                           size_t cap_out, size_t* bad_index);
/* The same with the columns and the output in host memory (N elements each; the range's cosets are uploaded, the device
   path runs, the range is downloaded; `out` outside the range is not written).  (src/config.rs:232-568) */
int lemsm_gate_eval(lemsm_ctx* ctx, const lemsm_gate_program* prog, const uint64_t* const* columns, size_t ncols, uint32_t logn, uint32_t logm,
                    uint32_t coset_begin, uint32_t coset_count, const uint64_t* shift, const uint64_t y[4], uint64_t* out, size_t cap_out,
                    size_t* bad_index);

/* ---- permutation and lookup grand products on resident columns (src/config.rs:228) --------------------------
   The product columns z of halo2's permutation and lookup arguments, built from columns resident in HBM.  bn256::Fr,
   32-byte raw Montgomery elements, the conventions of the lemsm_fft* / lemsm_gate* entries: LEMSM_ERR_BAD_ARG leaves
   nothing queued and the outputs untouched, field arguments must be canonical, the figures of every call go to
   lemsm_poly_last, option ws_canary guards every carved workspace.  Field multiplication is exact, so the host entry, the
   device entry and repeated calls give the same bytes whatever the association of the products.  The mapping to
   halo2_proofs' plonk/permutation/prover.rs and plonk/lookup/prover.rs is stated from memory; the formulas here are the
   contract. */
/* Pure host: the geometry of the engine's scan for n terms (tests size their cases by it).  tile: terms one block of the
   batched inversion owns; segment: consecutive terms one thread of the scan multiplies up; block_segments: up to this many
   segments the one scanning block takes one per thread, beyond it several.  n >= 2^40: LEMSM_ERR_BAD_ARG. */
int lemsm_fraction_products_geometry(size_t n, size_t* tile, size_t* segment, size_t* block_segments);
/* The engine: running products of fractions.  d_num: n_num device pointers, d_den: n_den device pointers (each count
   0 .. 8, an empty product is 1), n elements each, n arbitrary.  Term i is f_i = prod_j num_j[i] / prod_j den_j[i];
   d_out[r] = init prod_{i < r} f_i for r = 0 .. n - 1, so d_out[0] = init; init == NULL means 1.  d_out may be NULL.
   out_tap (4 limbs, optional) = d_out[tap] for tap < n and init prod_{i < n} f_i for tap == n; tap > n: LEMSM_ERR_BAD_ARG.
   n == 0 is LEMSM_OK with out_tap = init.
   A row i < n whose denominators multiply to zero is LEMSM_ERR_DIVISION_BY_ZERO, whatever its numerator: the lowest such
   i goes to *bad_index (optional) and lemsm_last_bad_index; d_out is not written and out_tap is not set.  halo2's batch_invert
   would leave the zero in place and z would die silently; here it is an error, as in lemsm_fraction_sums.  A zero
   numerator is legal: the products are 0 from there on.
   More than 8 columns on a side, a null column, init not canonical, or d_out overlapping the bytes of any input column:
   LEMSM_ERR_BAD_ARG.
   This is halo2's lookup product z[i+1] = z[i] (A_i + beta)(S_i + gamma) / ((A'_i + beta)(S'_i + gamma)) once the caller
   has formed the four factor columns; the permuted columns A', S' come from lemsm_lookup_permute_device below.
   lemsm_poly_last: bytes = 32 n (n_num + n_den + (d_out ? 1 : 0)); the products of the shipped kernels. */
int lemsm_fraction_products_device(lemsm_ctx* ctx, const void* const* d_num, size_t n_num, const void* const* d_den, size_t n_den, size_t n,
                                   const uint64_t* init, void* d_out, size_t tap, uint64_t* out_tap, size_t* bad_index);
/* The same with the columns and `out` (may be NULL) in host memory. */
int lemsm_fraction_products(lemsm_ctx* ctx, const uint64_t* const* num, size_t n_num, const uint64_t* const* den, size_t n_den, size_t n,
                            const uint64_t* init, uint64_t* out, size_t tap, uint64_t* out_tap, size_t* bad_index);
/* The witness part of halo2's permutation::Argument::commit (the reference's circuit enables equality on column c,
   src/config.rs:228).  n = 2^logn rows (logn 0 .. 26), ncols <= 64 value columns v_j and permutation columns sigma_j of n
   Lagrange values each, w = lemsm_fft_omega(logn), challenges beta, gamma and the coset multiplier delta (4 limbs each),
   chunk_len >= 1 columns per set and the tap row u < n.  Set s covers columns s chunk_len ..
   min(ncols, (s + 1) chunk_len) - 1; nsets = ceil(ncols / chunk_len).  The term of set s at row i is
     f_{s,i} = prod_j (v_j[i] + beta delta^j w^i + gamma) / prod_j (v_j[i] + beta sigma_j[i] + gamma),
   j the column's index over ALL columns (delta^j carries across sets), and the product columns are
     z_s[r] = init_s prod_{i < r} f_{s,i},  r = 0 .. n - 1,   init_0 = 1,  init_{s+1} = z_s[u].
   Rows above u hold the continued product; halo2 overwrites them with blinding values, and so does the caller.
   Pure host: validates (logn, ncols, chunk_len) and prices a call.  bytes = 32 n (2 ncols + nsets): every input column is
   read once by the shipped kernels and every z written once (the engine's own workspace traffic is not in it);
   field_mults: the products of the shipped kernels, per set of c columns n (4 c - 2 + (logn > 8) + (logn > 16) + 6) and
   the batched inversion and scan of DESIGN 7f; workspace_bytes: what a call reserves.  ncols == 0 gives zeros. */
int lemsm_permutation_plan(uint32_t logn, size_t ncols, size_t chunk_len, size_t* nsets, uint64_t* bytes, uint64_t* field_mults,
                           uint64_t* workspace_bytes);
/* d_values, d_sigmas: ncols device pointers each; d_z: nsets device pointers of n elements each; out_taps (nsets x 4 limbs,
   optional) = z_s[u].  A row whose denominators multiply to zero: LEMSM_ERR_DIVISION_BY_ZERO with *bad_index (optional) and
   lemsm_last_bad_index = s n + i of the first one (sets in order, the lowest row of the first failing set); the z columns of
   the sets before s are written, z_s and those behind it are not, and nothing but the index is defined then.  ncols == 0 is LEMSM_OK with nothing written.  chunk_len == 0, u >= n, a limit exceeded, a null
   pointer, beta / gamma / delta not canonical, or a d_z buffer overlapping any input column or another d_z:
   LEMSM_ERR_BAD_ARG.  The sets hang on each other through z_s[u]: a host loop with one 32-byte read-back per set.
   lemsm_poly_last reports the plan's figures and the summed device time of the sets. */
int lemsm_permutation_product_device(lemsm_ctx* ctx, const void* const* d_values, const void* const* d_sigmas, size_t ncols, uint32_t logn,
                                     const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta[4], size_t chunk_len, size_t usable_row,
                                     void* const* d_z, uint64_t* out_taps, size_t* bad_index);
/* The same with the columns and the z columns in host memory (uploaded, the device path, downloaded). */
int lemsm_permutation_product(lemsm_ctx* ctx, const uint64_t* const* values, const uint64_t* const* sigmas, size_t ncols, uint32_t logn,
                              const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta[4], size_t chunk_len, size_t usable_row,
                              uint64_t* const* z, uint64_t* out_taps, size_t* bad_index);

/* ---- lookup argument: sorted field elements and the permuted columns A', S' on resident columns -------------
   The step of halo2's lookup argument in front of its grand product: permute_expression_pair of plonk/lookup/prover.rs
   (stated from memory; the formulas here are the contract).  The reference's own lookup is the log-derivative one
   (src/config.rs:402-437); its running sums are lemsm_fraction_sums*.  bn256::Fr, 32-byte raw Montgomery elements, assumed
   canonical and not checked; the conventions of the lemsm_fft* / lemsm_gate* / lemsm_permutation* entries:
   LEMSM_ERR_BAD_ARG leaves nothing queued and the outputs untouched, the figures of every call go to lemsm_poly_last, option
   ws_canary guards every carved workspace.
   ORDER is the order of the standard-form integers raw R^-1 mod r (Ord on halo2's field type), NOT the order of the raw
   limbs.  The outputs are unique functions of the inputs (equal keys are identical bytes), so the host entry, the device
   entry and repeated calls give the same bytes.
   Pure host: the geometry of the sort (tests size their cases by it).  digit_bits: bits of one radix digit; tile: keys one
   block of a pass takes; max_passes = 256 / digit_bits: the passes of a sort none of which is skipped.  A digit position at
   which all n keys agree is skipped: a column of values below 2^16 sorts in 16 / digit_bits passes.  n > 2^28:
   LEMSM_ERR_BAD_ARG. */
int lemsm_sort_field_geometry(size_t n, uint32_t* digit_bits, size_t* tile, uint32_t* max_passes);
/* Pure host: prices one lemsm_lookup_permute_device call of n rows with no pass skipped.  bytes = 32 n (4 + 3 passes + 8)
   with passes = 2 max_passes (see lemsm_lookup_permute_device); workspace_bytes: what a call reserves.  n == 0 gives zeros,
   n > 2^28: LEMSM_ERR_BAD_ARG. */
int lemsm_lookup_permute_plan(size_t n, uint64_t* bytes, uint64_t* workspace_bytes);
/* d_out[0 .. n) = d_in[0 .. n) in ascending ORDER, in Montgomery form again.  n arbitrary, 0 .. 2^28 (more: LEMSM_ERR_BAD_ARG);
   n == 0 is LEMSM_OK.  d_out must not overlap d_in; a null pointer with n > 0: LEMSM_ERR_BAD_ARG.
   A key-only least-significant-digit-first radix sort of the standard-form keys, every pass stable.
   lemsm_poly_last: ms; bytes = the key bytes of the kernels that ran: 32 n (2 + 3 passes_run), and 32 n 2 more when no
   pass ran (the tile tables of a pass, 1 / 32 of its keys, are not in it); field_mults = 2 n, the two form conversions. */
int lemsm_sort_field_device(lemsm_ctx* ctx, const void* d_in, size_t n, void* d_out);
/* The same with `in` and `out` in host memory. */
int lemsm_sort_field(lemsm_ctx* ctx, const uint64_t* in, size_t n, uint64_t* out);
/* halo2's permute_expression_pair on the first n rows (n = the usable rows; the caller blinds the rest) of the compressed
   input column A = d_input and table column S = d_table:
     A' = d_input_perm is A in ascending ORDER.  Row r of A' is a HEAD when r == 0 or A'[r] != A'[r-1], else a REPEAT.
     S' = d_table_perm: S'[r] = A'[r] at every head, and one instance of that value leaves the multiset of S.  What is left
     of that multiset, in ascending ORDER, is L[0 .. R), R the number of repeats; the repeat of ascending rank j gets
     L[R - 1 - j].  (halo2: the leftovers in BTreeMap order, each popped onto the last remaining repeated row.)
   So A'[0] = S'[0], (A'[r] - S'[r]) (A'[r] - A'[r-1]) = 0 for r >= 1, and both pairs are equal as multisets: the lookup
   product of lemsm_fraction_products_device over (A + beta)(S + gamma) / ((A' + beta)(S' + gamma)) is exactly 1 at tap n.
   A value of A that is not in S: LEMSM_ERR_NOT_IN_TABLE (halo2: Error::ConstraintSystemFailure); *bad_index (optional) and
   lemsm_last_bad_index = the lowest row of A that holds the SMALLEST missing value; the outputs are not written.
   Rows >= n of both outputs are not written.  n == 0 is LEMSM_OK.  An output overlapping an input or the other output, a
   null pointer (n > 0), n > 2^28: LEMSM_ERR_BAD_ARG.
   lemsm_poly_last: ms; bytes = 32 n (4 + 3 passes_run + 8): the two conversions, the passes that ran of both sorts, and the
   key traffic of the S' kernels with the leftovers priced at n (their u32 flag and offset words are not in it);
   field_mults = 4 n, the two form conversions of both columns. */
int lemsm_lookup_permute_device(lemsm_ctx* ctx, const void* d_input, const void* d_table, size_t n, void* d_input_perm, void* d_table_perm,
                                size_t* bad_index);
/* The same with all four columns in host memory. */
int lemsm_lookup_permute(lemsm_ctx* ctx, const uint64_t* input, const uint64_t* table, size_t n, uint64_t* input_perm, uint64_t* table_perm,
                         size_t* bad_index);
/* The passes the last sort ran and skipped (run + skipped = max_passes); after lemsm_lookup_permute* summed over its two
   sorts (run + skipped = 2 max_passes). */
int lemsm_sort_last(const lemsm_ctx* ctx, uint32_t* passes_run, uint32_t* passes_skipped);
/* Pure host, no context: the two sizes above which a sort or a permuted pair takes another path (tests size their cases by
   them; both outputs optional).  convert_keys_per_trip: the keys one trip of the conversion's grid-stride loop takes; a column
   of more keys takes a second trip.  scan_top_words: the words above which the single block on top of the exclusive scan
   takes more than one block sum per thread; the tile table of a sort has 2^digit_bits words per tile, the flag scan of a
   permuted pair 2 n + 1.  Both are multiples of the geometry's tile. */
int lemsm_debug_sort_thresholds(size_t* convert_keys_per_trip, size_t* scan_top_words);

/* ---- log-derivative lookup: the multiplicity column m on resident columns (src/config.rs:402-437) -----------
   The reference's lookup argument states c[i+1] - c[i] = 1 / (v - b[i+1]) on the lookup rows and c[0] - c[-1] =
   -b[0] / (v - t[0]) on the table rows (:421-424): cell b[0] of a table row is the MULTIPLICITY of that table entry.  The two
   running sums are lemsm_fraction_sums*; this is the column that makes them meet.  The same column is m(X) of the halo2 forks
   with the log-derivative ("mv") lookup, where several input expressions share one table (stated from memory; the formula
   here is the contract).  The conventions of the lookup section above: bn256::Fr, 32-byte raw Montgomery elements, assumed
   canonical and not checked; ORDER is the order of the standard-form integers; LEMSM_ERR_BAD_ARG leaves nothing queued and
   the outputs untouched; the figures of every call go to lemsm_poly_last; option ws_canary guards every carved workspace.
     Column c of the k input columns has lens[c] rows; position sum_{c' < c} lens[c'] + r of their concatenation A[0 .. N) is
     row r of column c.  The table is T[0 .. t).
     m[j] = the number of positions i with A[i] == T[j] if j is the LOWEST row of T that holds that value, else 0.
   So sum_j m[j] = N, and for every v outside T: sum_i 1 / (v - A[i]) = sum_j m[j] / (v - T[j]).
   The output is a unique function of the inputs: the host entry, the device entry and repeated calls give the same bytes.
   Pure host: prices one call with no pass skipped.  bytes = 32 (3 N + 6 t + 3 max_passes (N + t)), field_mults = N + 3 t (see
   lemsm_lookup_multiplicities_device); N == 0: bytes = 32 t, field_mults = 0.  workspace_bytes: what a call reserves (0 when
   N == 0).  N == t == 0 gives zeros.  Every output is optional.  The refusals of the entry that need no pointer: k == 0,
   k > 16, lens == NULL, N or t above 2^28: LEMSM_ERR_BAD_ARG. */
int lemsm_lookup_multiplicities_plan(const size_t* lens, size_t k, size_t t, uint64_t* bytes, uint64_t* field_mults,
                                     uint64_t* workspace_bytes);
/* d_out_m[0 .. t) = m as 32-byte elements: form LEMSM_FORM_MONTGOMERY writes each count as a raw Montgomery element (what
   column b holds and what lemsm_fraction_sums_device takes as d_num), LEMSM_FORM_CANONICAL as a standard-form little-endian
   integer (the scalars lemsm_msm_device takes); any other form: LEMSM_ERR_BAD_ARG.  Rows >= t are not written.
   k = 1 .. 16; every lens[c] >= 0, and a column of no rows may have a NULL pointer; N <= 2^28 and t <= 2^28, independent
   of each other.  N == 0 gives all-zero m; t == 0 with N == 0 is LEMSM_OK and writes nothing.
   A value of A that T lacks (every value when t == 0 < N): LEMSM_ERR_NOT_IN_TABLE; *bad_index (optional) and
   lemsm_last_bad_index = the lowest POSITION OF THE CONCATENATION that holds the SMALLEST missing value; the output is not
   written.
   k == 0, k > 16, a null pointer with rows behind it, the output overlapping the table or an input column, N or t above
   2^28: LEMSM_ERR_BAD_ARG.
   The k columns are converted into one buffer of N standard-form keys and sorted, the table likewise (key-only); every
   table row in its own order finds its value's run in the sorted table and the lowest row of a run wins (a minimum of row
   indices); m is zeroed, and every run of the sorted table writes the length of its value's run in the sorted inputs to the
   winner's row.
   lemsm_sort_last: passes run and skipped, summed over the sorts the call ran (the inputs' when N > 0, the table's when N > 0
   and t > 0: run + skipped = max_passes times that number).
   lemsm_poly_last: ms; bytes = 32 (3 N + 6 t + 3 (N passes_run_inputs + t passes_run_table)): the conversions, the passes that
   ran, As read for the missing values, T read for the lowest rows, m zeroed, the sorted table read and the counts written
   priced at t (the probes of the binary searches and the u32 words are
   not in it); field_mults = N + 3 t as the plan prices them (the conversions, each table row's standard form again, the counts to
   Montgomery form: priced at t and in both forms).  N == 0: bytes = 32 t, field_mults = 0. */
int lemsm_lookup_multiplicities_device(lemsm_ctx* ctx, const void* const* d_inputs, const size_t* lens, size_t k,
                                       const void* d_table, size_t t, int form, void* d_out_m, size_t* bad_index);
/* The same with every column in host memory. */
int lemsm_lookup_multiplicities(lemsm_ctx* ctx, const uint64_t* const* inputs, const size_t* lens, size_t k,
                                const uint64_t* table, size_t t, int form, uint64_t* out_m, size_t* bad_index);

/* ---- challenge post-processing helpers (src/config.rs:166-187) ------------------------ */
/* Host-side (a handful of field operations each); field elements are raw Montgomery limbs of the BASE field of `curve`.
   to_curve_x (:166-175): returns c itself when c^3 + b is a square; the reference's loop never changes x (:170-173), so
   for a non-residue it spins forever: LEMSM_ERR_WOULD_NOT_TERMINATE.
   y_from_x (:177-182): the second component of sqrt_alt(x^3 + b): a square root when there is one (*is_square = 1), else
   sqrt(ROOT_OF_UNITY * (x^3 + b)) (*is_square = 0), as ff::Field::sqrt_alt specifies.  Which of the two roots: the one
   Tonelli-Shanks seeded with ROOT_OF_UNITY produces (a^((p+1)/4) for p = 3 mod 4); the upstream source is not in the
   reference tree, so the sign convention is parity-unpinned -- the other root is the negation.
   slope (:184-187): 3 x^2 / (2 y); y == 0 is the reference's invert().unwrap() panic: LEMSM_ERR_DIVISION_BY_ZERO. */
int lemsm_to_curve_x(int curve, const uint64_t c[4], uint64_t out_x[4]);
int lemsm_y_from_x(int curve, const uint64_t x[4], uint64_t out_y[4], int* is_square);
int lemsm_slope(int curve, const uint64_t xy[8], uint64_t out[4]);

/* ---- precompute_multiplicities ------------------------------------------------------- */
/* out[(k-1)] = k * pt for k = 1..base-1 (Jacobian), for each of n points:
   out_jacobian[(j*(base-1) + (k-1))*12 .. +12]. */
int lemsm_precompute_multiplicities(lemsm_ctx* ctx, int curve, const uint64_t* pts_jacobian, size_t n,
                                    uint8_t base, uint64_t* out_jacobian);

/* Same multiples as affine (x,y) pairs, out_affine[(j*(base-1) + (k-1))*8 .. +8]: the form
   src/config.rs:542-560 writes into the fixed table column (the reference inverts once per multiple,
   :550-554; here one batched inversion per input point). */
int lemsm_precompute_multiplicities_affine(lemsm_ctx* ctx, int curve, const uint64_t* pts_jacobian, size_t n,
                                           uint8_t base, uint64_t* out_affine);

/* ---- helpers ------------------------------------------------------------------------- */
/* Jacobian -> canonical comparison form: affine x||y, 32-byte little-endian canonical
   (non-Montgomery) integers; identity = 64 zero bytes. */
int lemsm_jacobian_to_canonical(int curve, const uint64_t jacobian[12], uint8_t out[64]);
/* Sum of `count` Jacobian points on the host (identity for count == 0).  Combines the partial
   results of an MSM whose POINTS were split across callers / GPUs -- the step halo2's
   best_multiexp performs over its per-thread chunk results (`results.iter().fold(identity, a + b)`
   in the halo2_proofs dependency the reference calls at src/argument_witness_calc.rs:144). */
int lemsm_jacobian_sum(int curve, const uint64_t* jacobian, size_t count, uint64_t out[12]);
/* Device memory helpers so that non-HIP hosts can stage resident inputs. */
int lemsm_device_alloc(lemsm_ctx* ctx, size_t bytes, void** out);
int lemsm_device_free(lemsm_ctx* ctx, void* p);
int lemsm_device_upload(lemsm_ctx* ctx, void* dst, const void* src, size_t bytes);
int lemsm_device_download(lemsm_ctx* ctx, void* dst, const void* src, size_t bytes);
/* P_i = (i+1) * Q on the device (affine, n x 8 limbs): synthetic bench/test inputs with a
   known discrete-log relation (sum s_i P_i == (sum s_i (i+1)) Q). */
int lemsm_device_gen_walk(lemsm_ctx* ctx, int curve, const uint64_t q_affine[8], size_t n, void* d_points_out);

/* ---- debug / known-answer hooks used by the parity tests ----------------------------- */
/* Raw Montgomery limbs (x * 2^256, canonical) in and out.  montmul: out = a*b*R^-1.  fieldop: 0 add, 1 sub, 2 neg(a),
   3 inverse(a) (Montgomery inverse), 4 sqr(a).  pointop: 0 = madd(acc XYZZ, q affine), 1 = add(acc XYZZ, q XYZZ),
   2 = madd_abi (the accumulate kernel's second form; an alias of 0 in the strict arithmetic).
   They run the arithmetic option "field" selects: 0, the default, is the lazy radix-2^29 field of the hot kernels
   (Field29 / XYZZ29; values enter through from_abi and leave through div32 + canon; op 3 is inv_lazy, the inversion of
   every batched-inversion kernel); 1 is the strict 32-bit-limb field.  Lazy field only: fieldop 5 = mul2(a, b, b, a) =
   2ab/R, 6 = sqr_addhi = a^2/R + b, 7 = mul_addhi = ab/R + b, 9 = mul32 round trip = a. */
int lemsm_debug_montmul(lemsm_ctx* ctx, int curve, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int lemsm_debug_fieldop(lemsm_ctx* ctx, int curve, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int lemsm_debug_pointop(lemsm_ctx* ctx, int curve, int op, const uint64_t* acc_xyzz, const uint64_t* q,
                        uint64_t* out_xyzz, size_t n);
/* Raw-limb entries of the lazy field (Field29) and its XYZZ law (XYZZ29): the inline functions the hot kernels call, on the
   limbs as they sit in registers, with no conversion in or out (option "field" plays no part).  n <= 2^24.
   field29_raw: a, b, c, d, n x 9 int32 each (pass zeros where an op has fewer operands); out n x 10 int32: the 9 result
   limbs, then a predicate word (1/0 for the boolean ops, 0 otherwise; their limbs echo a). */
enum {
  LEMSM_F29_MUL = 0,          /* mul(a, b) */
  LEMSM_F29_SQR = 1,          /* sqr(a) */
  LEMSM_F29_MUL2 = 2,         /* mul2(a, b, c, d) */
  LEMSM_F29_MUL_ADDHI = 3,    /* mul_addhi(a, b, hi = c) */
  LEMSM_F29_SQR_ADDHI = 4,    /* sqr_addhi(a, hi = c) */
  LEMSM_F29_ADD = 5,          /* add(a, b) */
  LEMSM_F29_SUB = 6,          /* sub(a, b) */
  LEMSM_F29_NEG = 7,          /* neg(a) */
  LEMSM_F29_CNEG = 8,         /* cneg(a, flag = b[0] != 0) */
  LEMSM_F29_WNORM = 9,        /* wnorm(a) */
  LEMSM_F29_CANON = 10,       /* canon(a) */
  LEMSM_F29_REDUCE_SMALL = 11,
  LEMSM_F29_MUL32 = 12,
  LEMSM_F29_FROM_ABI = 13,
  LEMSM_F29_DIV32 = 14,
  LEMSM_F29_IS_ZERO_MOD = 15, /* predicate */
  LEMSM_F29_LIMBS_ZERO = 16,  /* predicate */
  LEMSM_F29_HI_TERM = 17,     /* XYZZ29::hi_term(ppp = a, q = b) */
  LEMSM_F29_PP_IS_ZERO = 18,  /* XYZZ29::pp_is_zero(a), predicate */
  LEMSM_F29_SQR_SUBHI = 19    /* sqr_subhi(a, ppp = b, q = c) = a^2/R + 2N - b - 2c */
};
int lemsm_debug_field29_raw(lemsm_ctx* ctx, int curve, int op, const int32_t* a, const int32_t* b, const int32_t* c,
                            const int32_t* d, int32_t* out, size_t n);
/* xyzz29_raw: acc, q, out, n x 37 int32 each: 36 limbs (x, y, zz, zzz) and a flag word.  acc's flag is `empty` on entry to
   madd / madd_abi; out's flag is `empty` on exit, or add4_mem's return value (its record stays zero where it is 0).  madd and
   madd_abi take the incoming affine point from q's x and y; madd_abi runs on acc as given (the scaled form).  add4_mem runs
   as k_pyramid runs it: four lanes per pair, 16 pairs per wave, the record's 36-byte elements as its operands. */
enum {
  LEMSM_X29_MADD = 0,         /* madd(acc, q.x, q.y, empty) */
  LEMSM_X29_MADD_ABI = 1,     /* madd_abi(acc, q.x, q.y, empty) */
  LEMSM_X29_ADD = 2,          /* add(acc, q) */
  LEMSM_X29_DBL_AFFINE = 3,   /* dbl_impl<true>(acc) */
  LEMSM_X29_DBL = 4,          /* dbl_impl<false>(acc) */
  LEMSM_X29_SCALE = 5,
  LEMSM_X29_UNSCALE = 6,
  LEMSM_X29_ADD4_MEM = 7      /* add4_mem(acc, q) */
};
int lemsm_debug_xyzz29_raw(lemsm_ctx* ctx, int curve, int op, const int32_t* acc, const int32_t* q, int32_t* out, size_t n);
/* Plain transform over bn256::Fr of nseq sequences of 2^logn elements, natural order in and out, with the reference's
   omega = FftPrecomp::omega_pow(S - logn) (src/regular_functions_utils.rs:111-124); the inverse is scaled by 1/N. */
int lemsm_debug_ntt(lemsm_ctx* ctx, const uint64_t* in, uint64_t* out, size_t nseq, uint32_t logn, int inverse);
/* Self-test of the workspace guards (option "ws_canary": a 256-byte pattern behind every sub-buffer the library carves
   out of its device workspaces -- the MSM window group, the divisor-witness forest and its tables, the lhs / rhs witness
   and fraction-sum engines, the regular-function entries, lemsm_debug_ntt -- checked when the call's kernels have run; a
   damaged zone is LEMSM_ERR_HIP with "workspace guard <arena>/<block> overwritten at byte <k> (option ws_canary)" in
   lemsm_last_error).  Carves the blocks "first", "second", "third" of an arena "selftest" in the context's workspace,
   overwrites byte `byte` (< 256) of the zone behind block `which` (0..2; -1: none) with a memset and runs the check:
   LEMSM_ERR_HIP naming block and byte, LEMSM_OK for -1.  No kernel runs and nothing outside the workspace is written. */
int lemsm_debug_arena_selftest(lemsm_ctx* ctx, int which, uint32_t byte);
/* One-GPU rehearsal of the sharded entries: the pipelines of all `world` ranks run one after the other on this
   context and their record areas are placed where the all-gather would put them; everything but the ncclAllGather
   call itself is the code of lemsm_*_sharded_device. */
int lemsm_debug_msm_sharded_sim(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine, size_t n,
                                int world, uint64_t out_jacobian[12]);
int lemsm_debug_lhs_sharded_sim(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine, size_t n,
                                uint8_t base, int world, uint64_t out_carry[12], uint64_t* out_carries, size_t* bad_index);

#ifdef __cplusplus
}
#endif
#endif /* LEMSM_H */
