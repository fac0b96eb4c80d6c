/* h2agg.h — C ABI of libh2agg.so: the MI355X (gfx950) backend for the "pure calculation context" hot
 * path of scroll-tech/halo2-snark-aggregator.
 *
 * The reference has no FFI of its own (it is 100 % Rust).  The boundary this header
 * defines is the one a GPU-backed implementation of the reference's plugin traits would bind: every
 * entry point names the reference interface (file:line under /root/reference) whose arithmetic it
 * replaces.  The Rust-side binding a maintainer would add is shown in INTEGRATION.md and
 * halo2-snark-aggregator_amd/rust-shim/.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary, caller owns every buffer;
 *   - return 0 (H2AGG_OK) on success, otherwise an H2AGG_ERR_* code with a message available from
 *     h2agg_last_error(); the Mock chips cannot construct their generic error type `E`, they panic —
 *     the shim turns a non-zero status into a panic (mock/arith/field.rs:113, mock/arith/ecc.rs:128);
 *   - a context is bound to ONE device and is single-thread-affine (the reference's chips are used
 *     from one thread: SURVEY.md §8b); one context per (host thread, GPU);
 *   - there is NO CPU mode: creating a context without a usable HIP device fails (H2AGG_ERR_HIP).
 *
 * Encodings (all little-endian, canonical = fully reduced integer, NOT Montgomery form)
 *   FR / FQ      32 bytes, integer < modulus (what halo2curves `to_repr()` yields)
 *   G1 affine    x || y, 64 bytes; identity = 64 zero bytes      (halo2curves G1Affine, `C`)
 *   G1 jacobian  x || y || z, 96 bytes; identity has z = 0       (halo2curves G1, `C::CurveExt`)
 *   Jacobian outputs are a valid representative of the result point, not a canonical one: compare
 *   after h2agg_g1_batch_to_affine (the reference compares `to_affine()` values too,
 *   halo2-snark-aggregator-circuit/src/verify_circuit.rs:180,200).
 */
#ifndef H2AGG_H
#define H2AGG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct h2agg_ctx h2agg_ctx;

enum {
    H2AGG_OK = 0,
    H2AGG_ERR_INVALID = 1,      /* bad argument (null pointer, unknown op, bad handle, bad window size) */
    H2AGG_ERR_DIV_ZERO = 2,     /* inversion of zero: reference panics, mock/arith/field.rs:113 */
    H2AGG_ERR_EMPTY = 3,        /* multi_exp of zero pairs: reference panics, mock/arith/ecc.rs:128 */
    H2AGG_ERR_HIP = 4,          /* HIP runtime / device failure */
    H2AGG_ERR_NONCANONICAL = 5, /* an input integer was >= its modulus */
    H2AGG_ERR_NOMEM = 6,
    H2AGG_ERR_BAD_POINT = 7,    /* a compressed point does not decode: "invalid point encoding in proof", transcript.rs:65-70;
                                   a partial accumulator received from a peer rank is not on the curve */
    H2AGG_ERR_PEER = 8,         /* sharded aggregation: another rank failed (its code is in the message); this rank's inputs were fine */
    H2AGG_ERR_NOT_IN_TABLE = 9  /* h2agg_lookup_permute: an input value does not occur in the table (halo2: Error::ConstraintSystemFailure) */
};

/* field ops of h2agg_fr_batch_op */
enum { H2AGG_OP_ADD = 0, H2AGG_OP_SUB = 1, H2AGG_OP_MUL = 2, H2AGG_OP_SQR = 3, H2AGG_OP_INV = 4, H2AGG_OP_DIV = 5 };

/* ---- lifetime -------------------------------------------------------------------------------------
 * replaces: `MockEccChip::default()` / `MockFieldChip::default()` / `MockChipCtx::default()`
 * (halo2-snark-aggregator-circuit/src/verify_circuit.rs:115-118). */
int h2agg_create(int device_ordinal, h2agg_ctx** out);
void h2agg_destroy(h2agg_ctx* ctx);
const char* h2agg_last_error(const h2agg_ctx* ctx);
/* Use an existing HIP stream (hipStream_t) for every launch of this context; NULL = the context's own (a non-blocking stream:
 * it does NOT synchronise with the legacy default stream).  Device buffers handed to the asynchronous entry points must be
 * complete on THAT stream (or the device synchronised) before the call and must not change until the result has been joined:
 * the sort reads the scalars more than once.  Note that a framework's "default stream" usually has the handle 0 (= NULL here).
 * The call takes a few milliseconds: the context measures which of its other streams share a hardware queue with the new main
 * stream and hands their roles (tails, copies, ...) out again, so that none of them queues in front of the main stream's work. */
int h2agg_set_stream(h2agg_ctx* ctx, void* hip_stream);
/* Block until everything queued on the context's stream (and its tail streams) has finished.  Also where device-side
 * status raised by ASYNCHRONOUS calls surfaces: a non-canonical scalar handed to h2agg_g1_msm_device_async / _batch_async is
 * reported here (or by the next synchronous entry point, whichever comes first) as H2AGG_ERR_NONCANONICAL, once. */
int h2agg_synchronize(h2agg_ctx* ctx);
/* Library / device description, e.g. "h2agg 0.1 gfx950 cu=256"; valid until the context is destroyed. */
const char* h2agg_describe(h2agg_ctx* ctx);

/* ---- Fr batch ops (host buffers) ------------------------------------------------------------------
 * replaces: MockFieldChip::{add,sub,mul,square,div} element-wise over n operands
 * (halo2-snark-aggregator-api/src/mock/arith/field.rs:39-55, 98-122).  `b` is ignored for SQR / INV.
 * INV of 0 and DIV by 0 -> H2AGG_ERR_DIV_ZERO (reference: `invert().unwrap()` panics).  n == 0 is a no-op. */
int h2agg_fr_batch_op(h2agg_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out);
/* replaces: ArithFieldChip::pow_constant (arith/field.rs:83-104) over n bases with one exponent >= 1
 * (exponent 0 -> H2AGG_ERR_INVALID: the reference asserts). */
int h2agg_fr_batch_pow_constant(h2agg_ctx* ctx, const uint8_t* a, size_t n, uint64_t exponent, uint8_t* out);

/* replaces: ArithFieldChip::mul_add_accumulate default (Horner: acc = acc*b + v_i, acc_0 = 0)
 * (halo2-snark-aggregator-api/src/arith/field.rs:68-81). */
int h2agg_fr_mul_add_accumulate(h2agg_ctx* ctx, const uint8_t* v, size_t n, const uint8_t b[32], uint8_t out[32]);

/* replaces: MockFieldChip::sum_with_coeff_and_constant (acc = b + sum x_i*coeff_i)
 * (halo2-snark-aggregator-api/src/mock/arith/field.rs:124-135). */
int h2agg_fr_sum_with_coeff_and_constant(h2agg_ctx* ctx, const uint8_t* x, const uint8_t* coeff, size_t n,
                                         const uint8_t b[32], uint8_t out[32]);

/* ---- G1 batch ops (host buffers) ------------------------------------------------------------------
 * replaces: MockEccChip::add / sub (`*a + *b`, `*a - *b`) over n Jacobian pairs
 * (halo2-snark-aggregator-api/src/mock/arith/ecc.rs:30-46). */
int h2agg_g1_batch_add(h2agg_ctx* ctx, const uint8_t* a_jac, const uint8_t* b_jac, size_t n, int subtract,
                       uint8_t* out_jac);

/* replaces: MockEccChip::scalar_mul / scalar_mul_constant (`rhs * lhs`) over n (affine base, scalar) pairs
 * (halo2-snark-aggregator-api/src/mock/arith/ecc.rs:88-104); also the loop body of
 * assign_instance_commitment (halo2-snark-aggregator-api/src/systems/halo2/verify.rs:623-635). */
int h2agg_g1_batch_scalar_mul(h2agg_ctx* ctx, const uint8_t* bases_aff, const uint8_t* scalars, size_t n,
                              uint8_t* out_jac);

/* replaces: MockEccChip::to_value = `to_affine` (halo2-snark-aggregator-api/src/mock/arith/ecc.rs:64-66). */
int h2agg_g1_batch_to_affine(h2agg_ctx* ctx, const uint8_t* in_jac, size_t n, uint8_t* out_aff);

/* h2agg_g1_batch_to_affine for Jacobian points already in device memory (e.g. the outputs of
 * h2agg_g1_msm_device_async: N instance-column commitments become affine with one launch and one download). */
int h2agg_g1_batch_to_affine_device(h2agg_ctx* ctx, const uint8_t* d_in_jac, size_t n, uint8_t* out_aff);
/* ---- proof wire format (the data format on the input side of the path) ----------
 * replaces: the `C::from_bytes(&compressed)` of TranscriptRead::read_point / read_constant_point
 * (halo2-snark-aggregator-api/src/systems/halo2/transcript.rs:56-99), for all the points of a proof (or of N proofs) at once.
 * Encoding: 32 bytes little-endian x, parity of y in bit 7 of byte 31, identity = 32 zero bytes (halo2curves 0.2.1, recalled
 * from upstream: the crate is not vendored in the reference).  out_aff: canonical affine, 64 B each; ok (optional): one byte
 * per point, 1 = decoded.  Any point that does not decode (x >= p, or x^3 + 3 not a square) -> H2AGG_ERR_BAD_POINT with that
 * point's output zeroed and ok = 0; the others are still written. */
int h2agg_g1_batch_decompress(h2agg_ctx* ctx, const uint8_t* in, size_t n, uint8_t* out_aff, uint8_t* ok);
/* the inverse (G1Affine::to_bytes): canonical affine points -> 32-byte encodings */
int h2agg_g1_batch_compress(h2agg_ctx* ctx, const uint8_t* aff, size_t n, uint8_t* out);
/* Sum of n Jacobian points (the local fold after the multi-GPU all-gather of partial (W_x, W_g),
 * SURVEY.md §8e; arithmetic = MockEccChip::add, mock/arith/ecc.rs:30-37).  n == 0 -> identity. */
int h2agg_g1_sum(h2agg_ctx* ctx, const uint8_t* in_jac, size_t n, uint8_t out_jac[96]);

/* Page-locked host memory for the buffers handed to the host-buffer entry points (h2agg_g1_msm, h2agg_eval_flat, ...):
 * from pageable memory the 96 B/point cross PCIe through the runtime's bounce buffers (~15 GB/s); from these buffers the
 * copies run at link rate and asynchronously.  A binding marshals its points / scalars straight into them. */
int h2agg_host_alloc(h2agg_ctx* ctx, size_t bytes, void** out);
int h2agg_host_free(h2agg_ctx* ctx, void* p);
/* ---- multi-scalar multiplication ------------------------------------------------------------------
 * replaces: MockEccChip::multi_exp / ArithEccChip::multi_exp default — sum_i scalars[i] * bases[i]
 * (halo2-snark-aggregator-api/src/mock/arith/ecc.rs:106-129, .../arith/ecc.rs:42-60), called from
 * EvaluationQuerySchema::eval (halo2-snark-aggregator-api/src/systems/halo2/evaluation.rs:197).
 * The reference computes n independent double-and-add products; this computes the same group element
 * with a Pippenger bucket method on the GPU.  n == 0 -> H2AGG_ERR_EMPTY (the reference panics); the
 * output buffer is then set to the identity so a caller that prefers "empty sum = identity" can
 * ignore that one status. */
int h2agg_g1_msm(h2agg_ctx* ctx, const uint8_t* bases_aff, const uint8_t* scalars, size_t n, uint8_t out_jac[96]);
/* The same with the points as the trait hands them over: `Vec<C::CurveExt>`, projective (x || y || z, 96 B each, canonical;
 * z = 0: identity).  They are normalised on the device (one inversion per 8 points per lane), so the binding does not
 * have to run `batch_normalize` over a million points on one host core first (mock/arith/ecc.rs:106-129 takes
 * `points: Vec<Self::AssignedPoint>` = `C::CurveExt`); 128 instead of 96 bytes per point cross PCIe. */
int h2agg_g1_msm_jac(h2agg_ctx* ctx, const uint8_t* points_jac, const uint8_t* scalars, size_t n, uint8_t out_jac[96]);
/* S independent multi_exps (mock/arith/ecc.rs:106-129) over the segments [seg_start[s], seg_start[s+1]) of one
 * host-side point / scalar array, one set of device launches (replaces S calls of h2agg_g1_msm: the many small multi_exp
 * calls a drop-in caller makes, and the 2N evaluation sides of h2agg_verify_proofs).  seg_start: S + 1 non-decreasing
 * offsets, seg_start[0] = 0, seg_start[S] = n.  out_jac: S x 96 B canonical Jacobian.  An empty segment -> H2AGG_ERR_EMPTY
 * (as h2agg_g1_msm for n == 0: the reference's acc.unwrap()); a scalar >= r -> H2AGG_ERR_NONCANONICAL.  Segments are taken
 * in groups of whole segments of up to 16384 points per set of launches (test key "seg_chunk"); a longer segment is an
 * ordinary multi_exp of its own. */
int h2agg_g1_msm_segmented(h2agg_ctx* ctx, const uint8_t* bases_aff, const uint8_t* scalars, size_t n,
                           const uint64_t* seg_start, size_t nseg, uint8_t* out_jac);

/* replaces: eval()'s flat tail — multi_exp over the entries that carry a scalar, then `pchip.add` of
 * every scalar-less point (halo2-snark-aggregator-api/src/systems/halo2/evaluation.rs:189-200).
 * has_scalar[i] != 0 marks entries with a scalar.  No scalar-carrying entry -> H2AGG_ERR_EMPTY. */
int h2agg_eval_flat(h2agg_ctx* ctx, const uint8_t* pts_aff, const uint8_t* scalars, const uint8_t* has_scalar,
                    size_t n, uint8_t out_jac[96]);

/* ---- device-resident bases / scalars (SRS-style fixed bases; inputs stay in HBM) ------------------
 * A base table lives on the device in Montgomery form (64 B / point).  Used for the instance-commitment
 * MSM against `params.g_lagrange` (halo2-snark-aggregator-api/src/systems/halo2/verify.rs:623-635) and
 * for benchmarking with inputs already resident. */
int h2agg_bases_upload(h2agg_ctx* ctx, const uint8_t* bases_aff, size_t n, uint64_t* handle_out);
/* Fixed-base acceleration of a resident table (an SRS such as ParamsKZG.g_lagrange, the bases of
 * assign_instance_commitment, verify.rs:574-649): stores 2^(c*w) * P_i for every digit position w beside the table
 * (ceil(255 / c) x 64 B per point).  Every later MSM over this handle (h2agg_g1_msm_preloaded / _device / _device_async /
 * _device_batch_async, h2agg_instance_commitment) then drops all digits of a scalar into ONE bucket set: one bucket
 * reduction instead of one per window, no doubling chain, and a wider window.  window_bits: 0 = chosen from the table
 * size, else 4..20.  Tables up to ~2^18 points (ceil(255 / c) * n <= 2^22) take the width that minimises the work; larger
 * ones, up to 2^22 points, take c = 20: 13 levels = 832 B per point beside the table — 3.25 GiB for a 2^22-point g_lagrange,
 * built in ~80 ms — and a (level, point) sort of their own (csrc/fb_sort_kernels.hpp).  An explicit width other than 20 whose
 * levels exceed 2^22 entries, and tables beyond 2^22 points, are refused (H2AGG_ERR_INVALID) and keep the ordinary path.
 * window_bits = 0 is the opportunistic call: it returns H2AGG_ERR_NOMEM (table untouched, ordinary path kept) when the
 * levels would take more than a quarter of the device memory that is free; an explicit width allocates regardless.
 * Results are the same points (h2agg_msm_configure's explicit window_bits disables the fast path).  The c = 20 levels are
 * used by MSMs their own sort takes — one MSM at a time (batches of >= 2^18 scalars run one after another), no sort /
 * segment knobs configured; any other call over such a table runs the ordinary path and ignores the levels. */
int h2agg_bases_precompute(h2agg_ctx* ctx, uint64_t bases_handle, int window_bits);
/* bases[i] = k_i * G for n canonical Fr scalars held in DEVICE memory (workload generation: the
 * expected MSM is then (sum k_i * s_i) * G).  Arithmetic = scalar_mul_constant + to_affine. */
int h2agg_bases_generate(h2agg_ctx* ctx, const void* d_k_scalars, size_t n, uint64_t* handle_out);
int h2agg_bases_download(h2agg_ctx* ctx, uint64_t handle, size_t first, size_t n, uint8_t* out_aff);
int h2agg_bases_free(h2agg_ctx* ctx, uint64_t handle);

/* scalars in host memory, bases preloaded; uses the first n bases of the table */
int h2agg_g1_msm_preloaded(h2agg_ctx* ctx, uint64_t bases_handle, const uint8_t* scalars, size_t n,
                           uint8_t out_jac[96]);
/* replaces: the per-column body of assign_instance_commitment
 * (halo2-snark-aggregator-api/src/systems/halo2/verify.rs:601-603 bound, :623-635 sum inst_i * g_lagrange[i],
 * :637-640 identity for an empty column) against a preloaded `params.g_lagrange` table.  max_len =
 * params.n() - (blinding_factors + 1); len > max_len -> H2AGG_ERR_INVALID (the reference's assert!). */
int h2agg_instance_commitment(h2agg_ctx* ctx, uint64_t g_lagrange_handle, const uint8_t* instance, size_t len,
                              size_t max_len, uint8_t out_jac[96]);
/* scalars in DEVICE memory (n x 32 B canonical); synchronous, result to host */
int h2agg_g1_msm_device(h2agg_ctx* ctx, uint64_t bases_handle, const void* d_scalars, size_t n,
                        uint8_t out_jac[96]);
/* as above but asynchronous on the context's stream: the 96-byte canonical Jacobian result is written
 * to DEVICE memory at d_out_jac; nothing is copied to the host and the call does not synchronise. */
int h2agg_g1_msm_device_async(h2agg_ctx* ctx, uint64_t bases_handle, const void* d_scalars, size_t n,
                              void* d_out_jac);
/* `batch` MSMs over the SAME first n bases of the table, scalars laid out [batch][n] in device memory, results
 * d_out_jac[96 * q].  One set of launches computes all of them (the MSMs become extra windows of one bucket sort), so
 * many medium-sized MSMs fill the chip like one large one: the N instance-column commitments of N proofs against
 * ParamsKZG.g_lagrange (assign_instance_commitment, verify.rs:574-649) are this shape. */
int h2agg_g1_msm_device_batch_async(h2agg_ctx* ctx, uint64_t bases_handle, const void* d_scalars, size_t n, size_t batch,
                                    void* d_out_jac);

/* ---- EvaluationQuerySchema (the entry point of the hot path) ---------------------------------------
 * replaces: the AST of halo2-snark-aggregator-api/src/systems/halo2/evaluation.rs:15-27 and its
 * constructors `commit!` / `eval!` / `scalar!` (:41-60), `impl Add` / `impl Mul` (:62-84), `estimate`
 * (:295-330) and `eval` (:172-203, with eval_prepare :205-293).  A schema object is an arena of nodes
 * bound to one context; node ids are indices into it.  The host walks the tree exactly as eval_prepare
 * does but only records the schip.mul / schip.add calls on a tape; the tape runs on the GPU, its
 * results feed the multi_exp directly.  Keys are NUL-terminated strings (the reference's `String` keys). */
typedef struct h2agg_schema h2agg_schema;
int h2agg_schema_create(h2agg_ctx* ctx, h2agg_schema** out);
void h2agg_schema_destroy(h2agg_schema* s);
int h2agg_schema_node_commitment(h2agg_schema* s, const char* key, const uint8_t point_aff[64], uint32_t* node_out);
int h2agg_schema_node_eval(h2agg_schema* s, const uint8_t eval[32], uint32_t* node_out);     /* eval!(cq)   */
int h2agg_schema_node_scalar(h2agg_schema* s, const uint8_t scalar[32], uint32_t* node_out); /* scalar!(s)  */
int h2agg_schema_node_add(h2agg_schema* s, uint32_t l, uint32_t r, uint32_t* node_out);      /* l + r       */
int h2agg_schema_node_mul(h2agg_schema* s, uint32_t l, uint32_t r, uint32_t* node_out);      /* l * r       */
int h2agg_schema_estimate(h2agg_schema* s, uint32_t node, size_t* out);                      /* estimate(None) */
/* n x EvaluationQuery::new (evaluation.rs:100-118): nodes_out[i] = commit!(cq_i) + eval!(cq_i). */
int h2agg_schema_evaluation_queries(h2agg_schema* s, size_t n, const char* const* keys, const uint8_t* commitments,
                                    const uint8_t* evals, uint32_t* nodes_out);
/* Replace the commitment of an EvaluationQuery node created by h2agg_schema_evaluation_queries.  Lets the host build
 * the schema while the device is still computing that commitment (assign_instance_commitment's MSM,
 * verify.rs:574-649, whose result is the first query of every proof). */
int h2agg_schema_query_set_commitment(h2agg_schema* s, uint32_t query_node, const uint8_t point_aff[64]);
/* replaces: VerifierParams::get_point_schemas + batch_multi_open_proofs
 * (halo2-snark-aggregator-api/src/systems/halo2/multiopen.rs:23-102): queries (rotation, evaluation point,
 * schema node) in VerifierParams::queries order are grouped by rotation in first-seen order, Horner-folded
 * in v per group and in u over groups; `w` holds one W commitment per group (nw must equal the number of
 * groups — the reference's assert_eq!, multiopen.rs:48).  Keys of the W commitments: "{key}_w{i}". */
int h2agg_schema_batch_multi_open(h2agg_schema* s, const char* key, size_t nq, const int32_t* rotations,
                                  const uint8_t* points, const uint32_t* query_nodes, size_t nw, const uint8_t* w,
                                  const uint8_t v[32], const uint8_t u[32], uint32_t* w_x_out, uint32_t* w_g_out);
/* The Shplonk twin of h2agg_schema_batch_multi_open: the VERIFIER of the BDFG20 multiopen whose prover is
 * h2agg_kzg_shplonk_begin / _finish below, as a pair of schema nodes for h2agg_evaluate_multiopen_proof / _prepare.
 * Stands for: the verifier of poly/kzg/multiopen/shplonk (verifier.rs) and construct_intermediate_sets of halo2_proofs — an
 * unvendored git dependency of the reference: the set ordering and the order y, v, H1, u, H2 of a proof's tail are recalled
 * from upstream, not pinned; what is pinned is the definition in the Shplonk section below, which the
 * prover follows, and the verifier equation at its end.
 * Inputs: nq queries in VerifierParams::queries order, query q = (poly_ids[q], rotations[q], points + 32 q, query_nodes[q]);
 * the nodes are opaque, as for the GWC fold; H1, H2 canonical affine; y, v, u canonical scalars.
 *   A rotation names a point: the one the FIRST query of that rotation carries.  A polynomial's point set is the set of
 *   rotations its queries name; polynomials with equal point sets form set i, sets numbered in first-seen order of their first
 *   polynomial, polynomials p_{i,0}, p_{i,1}, ... inside a set in first-seen order of their first query; T: all rotations.
 *     l_{i,a}(u) = prod_{b in S_i, b != a} (u - z_b) / (z_a - z_b)                    (1 when |S_i| = 1)
 *     d_i = prod_{b in T \ S_i} (u - z_b),   c_i = d_i / d_0,   t = prod_{b in S_0} (u - z_b)   (= Z_T(u) / d_0)
 *     right = sum_i v^i c_i sum_j y^j sum_{a in S_i} l_{i,a}(u) * node(p_{i,j}, a)  +  (0 - t) * commit(H1)  +  u * commit(H2)
 *     left  = 1 * commit(H2)        (a scalar-carrying commitment: multi_exp of zero pairs is the reference's panic)
 *   Powers ascend from 0.  sum_a l_{i,a}(u) = 1: the commitment of p_{i,j} keeps the scalar v^i c_i y^j, the eval! parts of its
 *   nodes add up to r_{i,j}(u), which h2agg_evaluate_multiopen_proof subtracts as e G — the header's F + u H2.  Every scalar is
 *   recorded on the schema's Fr tape and computed on the device.  Keys of the two proof points: "{key}_shplonk_h1",
 *   "{key}_shplonk_h2".
 * Refusals (H2AGG_ERR_INVALID, the schema stays usable): an unknown node, nq == 0, a (polynomial, rotation) pair named twice,
 * a set of more than 32 points.  Two rotations with equal points, or u a point of T \ S_0, invert zero on the tape: the
 * EVALUATION returns H2AGG_ERR_DIV_ZERO.  y, v, u and points equal to 0 are legal, and so is u in S_0 (t = 0). */
int h2agg_schema_shplonk_multi_open(h2agg_schema* s, const char* key, size_t nq, const uint32_t* poly_ids,
                                    const int32_t* rotations, const uint8_t* points, const uint32_t* query_nodes,
                                    const uint8_t h1[64], const uint8_t h2[64], const uint8_t y[32], const uint8_t v[32],
                                    const uint8_t u[32], uint32_t* left_out, uint32_t* right_out);
/* eval(): out_jac = multi_exp(points with scalars) + sum(points without); *has_scalar / out_scalar = the
 * accumulated pure-scalar term (key ""), None -> *has_scalar = 0.  A Mul whose both sides hold
 * commitments, or an Add of non-singleton scalar sides, fails with H2AGG_ERR_INVALID (the reference's
 * assert!, evaluation.rs:237-238,282); no scalar-carrying commitment -> H2AGG_ERR_EMPTY (its panic). */
int h2agg_schema_eval(h2agg_schema* s, uint32_t node, uint8_t out_jac[96], int* has_scalar, uint8_t out_scalar[32]);
/* replaces: evaluate_multiopen_proof without the print-only pairing
 * (halo2-snark-aggregator-api/src/systems/halo2/verify.rs:705-731): left = eval(w_x) + e_x*G,
 * right = eval(w_g) - e_g*G, both `to_value`d; output order = verify_circuit_final_pair.data
 * (halo2-snark-aggregator-circuit/src/fs.rs:187-190). */
int h2agg_evaluate_multiopen_proof(h2agg_schema* s, uint32_t w_x, uint32_t w_g, uint8_t left_aff[64],
                                   uint8_t right_aff[64]);
/* The host half of h2agg_evaluate_multiopen_proof(s, w_x, w_g, ...) done ahead of time: both eval_prepare walks
 * (evaluation.rs:207-330) recorded on the Fr tape and the tape ordered by dependency level — no device work, no wait.
 * A following h2agg_evaluate_multiopen_proof with the same roots on an otherwise unchanged schema starts at the upload.
 * Commitment POINTS may still be replaced in between (h2agg_schema_query_set_commitment: the evaluation reads them
 * when it runs), so a host can prepare while the device is still computing the instance commitments (verify.rs:574-649).
 * Any other change to the schema (new nodes, another eval) simply makes the evaluation do its own host half again.
 * Same errors as the evaluation would report for the host half (H2AGG_ERR_INVALID, H2AGG_ERR_EMPTY). */
int h2agg_evaluate_multiopen_prepare(h2agg_schema* s, uint32_t w_x, uint32_t w_g);
/* names returned by the last eval (evaluation.rs:183) / points_wx ++ points_wg (verify.rs:711-712), and the
 * length MockChipCtx::point_list would have after the last multi_exp (mock/arith/ecc.rs:112-116). */
size_t h2agg_schema_name_count(h2agg_schema* s);
const char* h2agg_schema_name(h2agg_schema* s, size_t i);
/* all names in one call, each followed by '\n'; returns the byte count needed (nothing is written if cap is smaller) */
size_t h2agg_schema_names_joined(h2agg_schema* s, char* out, size_t cap);
size_t h2agg_schema_point_list_len(h2agg_schema* s);

/* ---- transcript side: Poseidon sponge, PoseidonEncode, PoseidonTranscriptRead ------------
 * replaces: PoseidonChip::{update, squeeze} (halo2-snark-aggregator-api/src/hash/poseidon.rs:167-191, permutation :193-230)
 * with T = 9, RATE = 8, R_F = 8, R_P = 63 (halo2-snark-aggregator-circuit/src/verify_circuit.rs:127-135), for `nproofs`
 * independent sponges at once (a sponge is a sequential chain; the batch is what runs in parallel).  elems: [nproofs][nelem]
 * canonical Fr; upto[q] = number of elements absorbed before squeeze q (non-decreasing, <= nelem; equal consecutive values
 * squeeze again without absorbing); out: [nproofs][nsq] challenges.  An element >= r -> H2AGG_ERR_NONCANONICAL. */
int h2agg_poseidon_squeeze_batch(h2agg_ctx* ctx, const uint8_t* elems, size_t nproofs, size_t nelem, const uint32_t* upto,
                                 size_t nsq, uint8_t* out);
/* replaces: PoseidonTranscriptRead (halo2-snark-aggregator-api/src/systems/halo2/transcript.rs:10-179) + PoseidonEncode
 * (mock/transcript_encode.rs:28-74) over `nproofs` proofs of ONE layout.  `script` is the sequence of calls the reader
 * receives, one character each: 'P' read_point, 'S' read_scalar, 'Q' squeeze_challenge_scalar, 'C' common_scalar(the next
 * of `consts`), 'X' common_point(the next of this proof's `ext_points_aff`, e.g. its instance commitments, verify.rs:77-97).
 * proof_len must equal 32 x (number of 'P' and 'S'): the reader's read_exact.  points_out: [nproofs][#P] decoded points
 * (canonical affine); challenges_out: [nproofs][#Q].  A point that does not decode -> H2AGG_ERR_BAD_POINT ("invalid point
 * encoding in proof"), a scalar >= r -> H2AGG_ERR_NONCANONICAL ("invalid field element encoding in proof"). */
/* The sponges are sequential chains (~136 permutations per proof): on the device a chain runs at one wave's latency whatever
 * the batch, on a host core ~an order of magnitude faster — so small batches run on host threads (one proof per thread, the
 * same generated constants, bit-identical challenges) and large ones on the device.  backend: 0 = auto (by batch size and
 * usable host threads; environment H2AGG_TRANSCRIPT=device|host overrides), 1 = device, 2 = host.  Applies to
 * h2agg_poseidon_squeeze_batch, h2agg_transcript_read_batch and h2agg_verify_aggregation(_ex) on this context.
 * h2agg_poseidon_squeeze_batch_host: the host backend on its own (no context, no device): max_threads 0 = all usable.
 * h2agg_host_threads: worker threads the library may use (affinity mask, cgroup CPU quota, H2AGG_HOST_THREADS; <= 32). */
int h2agg_transcript_configure(h2agg_ctx* ctx, int backend);
int h2agg_poseidon_squeeze_batch_host(const uint8_t* elems, size_t nproofs, size_t nelem, const uint32_t* upto, size_t nsq,
                                      uint8_t* out, int max_threads);
int h2agg_host_threads(void);
/* arithmetic of the host sponge: 1 = AVX-512 IFMA (chosen at run time when the CPU has avx512ifma), 0 = portable 4 x 64-bit.
 * In h2agg_poseidon_squeeze_batch_host, max_threads bit 16 forces the portable kernel and bit 17 the IFMA one for that call
 * (bits 0..15 stay the thread cap): the two are differential partners in tests/test_host_sponge.py. */
int h2agg_host_sponge_kind(void);
int h2agg_transcript_read_batch(h2agg_ctx* ctx, const uint8_t* proofs, size_t proof_len, size_t nproofs, const char* script,
                                size_t script_len, const uint8_t* consts, size_t nconsts, const uint8_t* ext_points_aff,
                                size_t next, uint8_t* points_out, uint8_t* challenges_out);
/* The second transcript family: ShaRead (halo2-snark-aggregator-api/src/transcript/sha.rs:23-127) over a digest D — SHA-256,
 * with which the OUTER proof of an aggregation is written and checked (ShaWrite at halo2-snark-aggregator-circuit/src/
 * verify_circuit.rs:985, VerifyCheck::call :1032-1055), or Keccak-256 (original padding 0x01 .. 0x80, rate 136; NOT SHA3-256),
 * from which the solidity code generator takes its challenges (halo2-snark-aggregator-solidity/src/transcript/codegen.rs:34,
 * 196-214).  A key's proofs are written with one transcript: its kind. */
#define H2AGG_TRANSCRIPT_KIND_POSEIDON 0
#define H2AGG_TRANSCRIPT_KIND_SHA256 1
#define H2AGG_TRANSCRIPT_KIND_KECCAK256 2
/* The ShaRead twin of h2agg_transcript_read_batch: the same scripts (P S Q C X) over `nproofs` proofs of one layout, kind =
 * H2AGG_TRANSCRIPT_KIND_SHA256 or _KECCAK256 (anything else -> H2AGG_ERR_INVALID).
 *   'P' read_point (sha.rs:43-61): 64 bytes, x then y, 32-byte little-endian each, uncompressed (no square root); a coordinate
 *       >= p ("invalid base encoding in proof"), a point off y^2 = x^3 + 3 — (0, 0) included — ("invalid point encoding in
 *       proof") -> H2AGG_ERR_BAD_POINT;
 *   'S' read_scalar (sha.rs:63-75): 32 bytes little-endian; >= r -> H2AGG_ERR_NONCANONICAL;
 *   'X' / 'C' common_point / common_scalar (sha.rs:94-126): absorb 31 zero bytes, 0x01, x and y big-endian (96 bytes) / 31 zero
 *       bytes, 0x02, the scalar big-endian (64 bytes); an external point that is the identity or not a canonical point of the
 *       curve ("cannot write points at infinity to the transcript") -> H2AGG_ERR_BAD_POINT;
 *   'Q' squeeze_challenge (sha.rs:81-92): absorb 0x00, digest = finalize(clone), the state restarts as D(digest), the
 *       challenge is the digest read as a little-endian integer mod r (Challenge255::new(digest | 32 zero bytes) = Fr::
 *       from_bytes_wide; halo2_proofs is unvendored in the reference: recalled).
 * proof_len must equal 64 x #P + 32 x #S (H2AGG_ERR_INVALID otherwise).  points_out: [nproofs][#P] canonical affine (zeros for
 * a point that was refused); challenges_out: [nproofs][#Q] canonical.  Backend as h2agg_transcript_configure / H2AGG_TRANSCRIPT
 * say (device: one lane per proof, state in registers; host: one proof per pool thread, portable SHA-256 / Keccak-256 inside
 * the library) — bit-identical; auto = host.
 * h2agg_hash_transcript_read_batch_host: the host backend on its own (no context, no device); max_threads 0 = all usable.
 * h2agg_hash_digest_host: D(msg) of the library's own host digests (what the tests pin against published vectors). */
int h2agg_hash_transcript_read_batch(h2agg_ctx* ctx, int kind, const uint8_t* proofs, size_t proof_len, size_t nproofs,
                                     const char* script, size_t script_len, const uint8_t* consts, size_t nconsts,
                                     const uint8_t* ext_points_aff, size_t next, uint8_t* points_out, uint8_t* challenges_out);
int h2agg_hash_transcript_read_batch_host(int kind, const uint8_t* proofs, size_t proof_len, size_t nproofs, const char* script,
                                          size_t script_len, const uint8_t* consts, size_t nconsts, const uint8_t* ext_points_aff,
                                          size_t next, uint8_t* points_out, uint8_t* challenges_out, int max_threads);
int h2agg_hash_digest_host(int kind, const uint8_t* msg, size_t len, uint8_t out[32]);

/* ---- verifier-params pipeline + aggregation driver (SURVEY.md 8(f) row 1 and the caller of the hot path) ----------
 * replaces, for the pure-calculation context: VerifierParamsBuilder::build_params (halo2-snark-aggregator-api/src/systems/
 * halo2/verify.rs:342-571), VerifierParams::queries (params.rs:74-224) with lagrange.rs / expression.rs / permutation.rs /
 * lookup.rs / vanish.rs, assign_instance_commitment (verify.rs:574-649), verify_aggregation_proofs_in_chip (verify.rs:
 * 835-942) and the pairing of calc_verify_circuit_final_pair (halo2-snark-aggregator-circuit/src/verify_circuit.rs:114-201).
 * The host replays the reference's control flow; every field / group operation runs on the device (instance MSMs, point
 * decompression, one Poseidon sponge per proof, ONE Fr tape for all expressions and eval_prepare scalars, the two
 * multi_exps).
 *
 * h2agg_vk: what the path reads of halo2_proofs' VerifyingKey / ConstraintSystem (unvendored), serialized little-endian:
 *   u32 magic 0x4B563248 ("H2VK"), u32 version 1,
 *   u32 k, num_advice_columns, num_instance_columns, num_challenges, degree (cs.degree()), blinding_factors,
 *   advice_column_phase: num_advice bytes; challenge_phase: num_challenges bytes           (each padded to 4 bytes)
 *   advice_queries, instance_queries, fixed_queries: u32 count, then (u32 column, i32 rotation) each
 *   permutation columns: u32 count, then (u32 kind: 0 advice / 1 fixed / 2 instance, u32 index) each
 *   fixed commitments: u32 count + 64 B each; permutation commitments: u32 count + 64 B each   (canonical affine)
 *   vk transcript scalar: 32 B  (from_bytes_wide(blake2b("Halo2-Verify-Key", pinned vk)), verify.rs:57-70)
 *   gates: u32 count; per gate u32 polys; per poly an expression;  lookups: u32 count; per lookup: u32 n + input
 *   expressions, u32 n + table expressions
 *   expression = u32 byte length + postfix bytecode (padded to 4): 0 CONST(32 B) 1 FIXED(u32 query index) 2 ADVICE(u32)
 *   3 INSTANCE(u32) 4 CHALLENGE(u32) 5 NEG 6 SUM 7 PRODUCT 8 SCALED(32 B)   (halo2_proofs::plonk::Expression; selectors
 *   are gone after keygen: expression.rs:33-35)
 * h2agg_circuit_proofs = CircuitProof (verify.rs:769-783): one verifying key with its proofs; every proof carries ONE
 * inner proof (instances[i] = that proof's instance columns back to back, instance_lens[i * num_instance_columns + col]
 * values each); all transcripts of a circuit have one length.  name: CircuitProof::name (keys are "{name}_p{i}").
 * g_lagrange: a base-table handle holding params.g_lagrange (h2agg_bases_upload; h2agg_bases_precompute speeds it up).
 * Outputs: the final pair (W_x, W_g) as fs.rs:187-190 lays it out; lambda_out (optional) = the aggregation challenge;
 * with s_g2 / g2 (both or none) *pairing_ok = e(W_x, s_g2) * e(W_g, -g2) == 1.
 * Errors: a proof point that does not decode -> H2AGG_ERR_BAD_POINT; a scalar >= r -> H2AGG_ERR_NONCANONICAL; a proof whose
 * length does not fit the key, a W count different from the number of rotation groups (multiopen.rs:48), an instance
 * column longer than n - (blinding_factors + 1) (verify.rs:601-603) -> H2AGG_ERR_INVALID; inversion of zero in the
 * Lagrange / vanishing terms -> H2AGG_ERR_DIV_ZERO (the reference's invert().unwrap()). */
typedef struct h2agg_vk h2agg_vk;
int h2agg_vk_create(h2agg_ctx* ctx, const uint8_t* blob, size_t len, h2agg_vk** out);
void h2agg_vk_destroy(h2agg_vk* vk);
/* The transcript the key's proofs are written with: H2AGG_TRANSCRIPT_KIND_POSEIDON (the default: every existing caller is
 * unchanged), _SHA256 or _KECCAK256 (ShaRead, sha.rs:23-127; above).  h2agg_verify_proofs honours it per circuit — one call
 * may mix kinds: proof points are 64 uncompressed bytes (sha.rs:53-54), so the length checks and the W count use 64-byte
 * points, the on-curve check replaces point decompression, and status / pairing_ok / advice_out work as for Poseidon (a
 * Poseidon-written proof under a SHA key does not fit the key's length: H2AGG_ERR_INVALID for that proof; an instance column
 * without values commits to the identity, which ShaRead refuses: H2AGG_ERR_BAD_POINT for that proof).
 * h2agg_verify_aggregation, _ex and _sharded return H2AGG_ERR_INVALID before any work when a key's kind is not Poseidon:
 * the reference never folds ShaRead proofs under an aggregation transcript (the outer proof is checked on its own,
 * verify_circuit.rs:1032-1055) — out of scope here. */
int h2agg_vk_set_transcript(h2agg_vk* vk, int kind);
/* The multiopen scheme the key's proofs end in: H2AGG_MULTIOPEN_GWC (the default: every existing caller is unchanged; the
 * proof ends in v, one W per rotation group, u — multiopen.rs:23-102) or H2AGG_MULTIOPEN_SHPLONK (halo2_proofs' ProverSHPLONK /
 * VerifierSHPLONK, which the reference does not read: recalled, not pinned — after the evaluations the proof reads y, v, H1, u,
 * H2 and is verified by h2agg_schema_shplonk_multi_open's definition, a query's polynomial being its commitment's key; the
 * vanishing query is a polynomial of its own).  Anything else -> H2AGG_ERR_INVALID.  The H2VK blob format is unchanged: the
 * kind is a switch on the parsed key, like the transcript kind, and may be changed between calls (a recording kept for the
 * other kind is not handed back).
 * h2agg_verify_proofs honours it per circuit — one call may mix GWC and Shplonk circuits; a Shplonk proof is exactly the
 * key's scalars and points plus H1 and H2, any other length -> H2AGG_ERR_INVALID for that proof (so a GWC proof under a
 * Shplonk key, or the reverse, whenever their lengths differ.  They coincide for a circuit whose queries name exactly two
 * rotations: its GWC proofs end in two W points.  Such a proof under a key of the other kind is read as that kind: status
 * H2AGG_OK and a pairing verdict of 0, not an error).  h2agg_verify_aggregation and _ex accept Shplonk keys and
 * mixed calls: the fold is linear in the pair whatever produced it; status, pairing_ok, advice_out and the plan cache work as
 * for GWC.  h2agg_verify_aggregation_sharded returns H2AGG_ERR_INVALID for a Shplonk key before any exchange — out of
 * scope for now. */
#define H2AGG_MULTIOPEN_GWC 0
#define H2AGG_MULTIOPEN_SHPLONK 1
int h2agg_vk_set_multiopen(h2agg_vk* vk, int kind);
typedef struct {
    const h2agg_vk* vk;
    const char* name;
    uint64_t g_lagrange;
    size_t nproofs;
    const uint8_t* const* transcripts;
    const size_t* transcript_lens;
    const uint8_t* const* instances;
    const uint32_t* instance_lens;
} h2agg_circuit_proofs;
int h2agg_verify_aggregation(h2agg_ctx* ctx, const h2agg_circuit_proofs* circuits, size_t ncircuits, const uint8_t* s_g2,
                             const uint8_t* g2, uint8_t left_aff[64], uint8_t right_aff[64], uint8_t lambda_out[32],
                             int* pairing_ok);
/* as above, plus the fourth return value of verify_aggregation_proofs_in_chip (`commits`: every proof's advice
 * commitments, halo2-snark-aggregator-api/src/systems/halo2/verify.rs:852-856,927-939, which the production caller hands to
 * `coherent`, halo2-snark-aggregator-circuit/src/verify_circuit.rs:487-492): advice_out (optional) receives, in aggregation
 * order, num_advice_columns x 64 B per proof (canonical affine, column order); advice_cap = bytes available (too small ->
 * H2AGG_ERR_INVALID before any work). */
int h2agg_verify_aggregation_ex(h2agg_ctx* ctx, const h2agg_circuit_proofs* circuits, size_t ncircuits, const uint8_t* s_g2,
                                const uint8_t* g2, uint8_t left_aff[64], uint8_t right_aff[64], uint8_t lambda_out[32],
                                int* pairing_ok, uint8_t* advice_out, size_t advice_cap);
/* The same aggregation with its proofs SHARDED over `world` ranks, one GPU each (first grain; BASELINE.json
 * configs[3], configs[4]).  This rank passes ITS proofs in `circuits` (any subset, typically round-robin; a rank may hold none)
 * and says where each sits in the aggregation order: global_index[j] for the j-th local proof, counting circuits in order and
 * proofs within a circuit in order; total_proofs = N, the length of the whole aggregation.  Two exchanges, both inside the call:
 *   1. every proof's last squeeze (32 B) goes to every rank, which absorbs them in aggregation order and squeezes the SAME
 *      lambda as the one-rank call (halo2-snark-aggregator-api/src/systems/halo2/verify.rs:909-913, :924);
 *   2. the rank's partial pair  sum_j lambda^(N-1-global_index[j]) * (W_x_j, W_g_j)  (the fold of verify.rs:926-938, which is
 *      linear) goes to every rank and is summed with the group law (RCCL has no reduction over group elements).
 * Transport: `allgather` (the host's own: MPI, a torch.distributed store, sockets — send = this rank's `bytes`, recv = [world]
 * [bytes] in rank order, returns 0) or, if NULL, the context's RCCL communicator over xGMI (h2agg_comm_init_rank with the same
 * rank / world).  Every rank returns the same pair, lambda and pairing verdict as h2agg_verify_aggregation on all N proofs in
 * one context, bit for bit.  advice_out: this rank's proofs only, local order.  Errors as h2agg_verify_aggregation; two ranks
 * claiming one position, or a position nobody holds -> H2AGG_ERR_INVALID on every rank.
 * No rank waits for a rank that failed: once its shard description is accepted a rank enters BOTH exchanges whatever happens
 * to it locally (a proof that does not decode, a non-canonical scalar, no memory, advice_cap too small) — each payload
 * carries a status word — and every rank leaves the call at the same exchange: the failing rank with its own error, the
 * others with H2AGG_ERR_PEER.  (A rank whose shard DESCRIPTION is refused — bad rank / world, repeated global_index, no
 * transport — returns before any exchange: that is a caller's bug, the same on every rank of a correct launch.)  Trust: the
 * squeezes and partial pairs of the other ranks arrive through the transport; partial pairs are checked to be canonical
 * points of the curve (H2AGG_ERR_NONCANONICAL / H2AGG_ERR_BAD_POINT), but a rank that LIES within those bounds changes the
 * result — ranks and transport are inside the verifier's trust boundary, as the threads of the reference's one process are. */
typedef int (*h2agg_allgather_fn)(void* user, const void* send, size_t bytes, void* recv);
typedef struct {
    uint32_t rank, world;
    size_t total_proofs;
    const uint32_t* global_index;
    h2agg_allgather_fn allgather;
    void* user;
} h2agg_shard;
int h2agg_verify_aggregation_sharded(h2agg_ctx* ctx, const h2agg_circuit_proofs* circuits, size_t ncircuits,
                                     const h2agg_shard* shard, const uint8_t* s_g2, const uint8_t* g2, uint8_t left_aff[64],
                                     uint8_t right_aff[64], uint8_t lambda_out[32], int* pairing_ok, uint8_t* advice_out,
                                     size_t advice_cap);
/* The host-side recording of an aggregation (every proof's queries of params.rs:74-224, the multiopen fold, both eval_prepare
 * walks of evaluation.rs:205-293) depends on the SHAPE of the call only — which keys, how many proofs of each, their length —
 * so a context keeps the last few recordings and a later call of the same shape only refills the proof scalars, challenges and
 * commitments before running the same tape and multi_exps on them (every value is still computed from that call's inputs).
 * This reports how often that happened; any pointer may be NULL.  h2agg_debug_configure(ctx, "plan_cache", 0) records every
 * call afresh. */
int h2agg_verify_plan_stats(h2agg_ctx* ctx, uint64_t* hits, uint64_t* misses, uint64_t* plans_kept);
/* verify_single_proof_in_chip (halo2-snark-aggregator-api/src/systems/halo2/verify.rs:779-833) for EVERY proof of
 * `circuits`, in one call: no aggregation challenge, no fold (verify_single_proof_no_eval, :651-688, then
 * evaluate_multiopen_proof, :690-745, per proof).  Per proof i (aggregation order: circuits in order, proofs in order):
 *   left_aff[64 i], right_aff[64 i]  that proof's evaluate_multiopen_proof pair, canonical affine;
 *   status[i]   H2AGG_OK, or THIS proof's error: H2AGG_ERR_BAD_POINT / H2AGG_ERR_NONCANONICAL (its bytes do not decode),
 *               H2AGG_ERR_INVALID (its transcript length does not fit the key, its W count != rotation groups,
 *               multiopen.rs:48, an instance column too long, verify.rs:601-603) — the other proofs are still verified;
 *   pairing_ok[i] (with s_g2 / g2, both or none) e(left_i, s_g2) * e(right_i, -g2) == 1; 0 when status[i] != OK.
 * The proofs of one circuit may differ in length here (each is checked against the key on its own).
 * advice_out / advice_cap as in h2agg_verify_aggregation_ex (the fourth return value of verify_single_proof_in_chip); a
 * proof whose status is not OK leaves zeros there.
 * Call-level errors only for the call itself: null buffers, no proofs, bad vk / table handle, H2AGG_ERR_NOMEM / _HIP,
 * and H2AGG_ERR_DIV_ZERO (one shared Fr tape; a zero denominator needs a challenge on a root of unity).
 * The common path is one set of launches for all proofs: the instance MSMs, transcripts and query recording of the
 * aggregation, then the 2N multi_exps as one segmented multi_exp (h2agg_g1_msm_segmented's kernels) and the N pairings on
 * the host pool.  When a proof's bytes do not decode, the proofs are verified again one by one to name it.  Per-proof
 * recordings are not kept in the aggregation's plan cache (h2agg_verify_plan_stats counts aggregation calls only). */
int h2agg_verify_proofs(h2agg_ctx* ctx, const h2agg_circuit_proofs* circuits, size_t ncircuits, const uint8_t* s_g2,
                        const uint8_t* g2, uint8_t* left_aff, uint8_t* right_aff, int32_t* status, int* pairing_ok,
                        uint8_t* advice_out, size_t advice_cap);
/* After h2agg_debug_configure(ctx, "phases", 1): the wall-clock split of the context's last h2agg_verify_aggregation* (or
 * h2agg_verify_proofs) call as
 * one line — " name=milliseconds" per phase in order, then the CPU the calling thread started and ended on and how often it was
 * preempted, then every host sponge chain's start offset, run time (microseconds) and CPU.  For latency reports (which phase a
 * slow call spent its time in); costs a few clock reads per call.  Owned by the context, valid until its next call.
 * After an h2agg_kzg_multiopen* call it is that call's split instead, from events on the context's stream:
 * " combine=ms divide=ms commit=ms" — the linear combinations, the up- and down-sweep over all groups, and the batch MSM with
 * the conversion to affine (this one includes the host's wait between the two).
 * After an h2agg_quotient* call it is that call's split, also from events on the stream and summed over the cosets:
 * " forward=ms gates=ms permutation=ms lookups=ms inverse=ms".
 * After h2agg_kzg_shplonk_begin / _finish it is that call's split, from events on the stream: " stage=ms numerators=ms divide=ms
 * commit=ms" (the slab's copy, the N_i, the sweeps and the set division summed over the sets, the MSM with its conversion) /
 * " combine=ms divide=ms commit=ms". */
const char* h2agg_last_phases(h2agg_ctx* ctx);

/* ---- multi-GPU exchange -----------------------------------------------------------
 * The one collective of a sharded aggregation: every rank holds partial accumulators (the sharded form of the fold
 * `acc = acc * lambda + proof`, halo2-snark-aggregator-api/src/systems/halo2/verify.rs:926-938, evaluated per shard);
 * they are all-gathered over RCCL / xGMI and summed with the group law on every rank (RCCL has no reduction over group
 * elements), for the caller halo2-snark-aggregator-circuit/src/verify_circuit.rs:114-201.  RCCL is dlopen'ed at the
 * first call.
 *   one process per GPU : rank 0 calls h2agg_comm_unique_id and hands the 128 bytes to the other ranks by the host's own
 *                         means; every rank calls h2agg_comm_init_rank on its context; then
 *                         h2agg_allgather_add_points(&ctx, 1, my_partials, npts, out).
 *   one process, N GPUs : h2agg_comm_create(devices, n, ctxs) creates the N contexts and their communicator
 *                         (ncclCommInitAll); h2agg_allgather_add_points(ctxs, n, partials[rank][npts], npts, out).
 * partial_jac: canonical Jacobian points (96 B); out_aff[64 * k] = to_affine(sum over ranks of point k), identical on
 * every rank.  The communicator is released by h2agg_destroy. */
int h2agg_comm_unique_id(uint8_t out[128]);
int h2agg_comm_init_rank(h2agg_ctx* ctx, const uint8_t id[128], int rank, int nranks);
int h2agg_comm_create(const int* devices, int ndev, h2agg_ctx** ctxs_out);
int h2agg_comm_size(h2agg_ctx* ctx);   /* 0 = no communicator */
int h2agg_comm_rank(h2agg_ctx* ctx);   /* -1 = no communicator */
/* why the last context-less comm call failed (h2agg_comm_unique_id, or h2agg_comm_create before a context exists):
 * e.g. the dlopen error of librccl.  Thread-local storage; valid until the thread's next call of this function. */
const char* h2agg_comm_last_error(void);
int h2agg_allgather_add_points(h2agg_ctx** ctxs, int nctx, const uint8_t* partial_jac, size_t npts, uint8_t* out_aff);

/* ---- pairing check (host arithmetic, no device work) ---------------------------
 * replaces: `E::multi_miller_loop(&[(&left_v, &s_g2_prepared), (&right_v, &n_g2_prepared)]).final_exponentiation()
 * .is_identity()` (halo2-snark-aggregator-api/src/systems/halo2/verify.rs:733-739) and the production assert
 * (halo2-snark-aggregator-circuit/src/verify_circuit.rs:175-199): BN254 optimal-ate pairing, exact final exponentiation.
 * Encodings: G1 affine as everywhere (64 B); G2 affine = x.c0 || x.c1 || y.c0 || y.c1 (128 B, canonical little-endian,
 * halo2curves G2Affine { x: Fq2 { c0, c1 }, y }; identity = 128 zero bytes).  Points are validated: coordinate >= p ->
 * H2AGG_ERR_NONCANONICAL; not on the curve / twist, or a G2 point outside the order-r subgroup -> H2AGG_ERR_BAD_POINT.
 * `ctx` only receives the error message and may be NULL.
 * h2agg_pairing_check: *ok = (prod_i e(g1_i, g2_i) == 1), the shape of EIP-197's precompile (n == 0 -> 1).
 * h2agg_pairing_product: the GT element itself, 12 x 32 B canonical in tower order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ...,
 *   c1.c2.c1; Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - (9 + u)), Fq2 = Fq[u]/(u^2 + 1)).
 * h2agg_final_pair_check: *ok = (e(left, s_g2) * e(right, -g2) == 1) — `params.s_g2()`, `params.g2()` as the caller
 *   holds them (ParamsKZG); the negation of g2 happens inside, as in the reference. */
int h2agg_pairing_check(h2agg_ctx* ctx, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, int* ok);
/* 64-byte compressed G2 points (how ParamsKZG::write stores `g2` / `s_g2`; read back at halo2-snark-aggregator-circuit/
 * src/fs.rs:49-55 through halo2_proofs) -> the 128-byte affine form above.  Encoding recalled from halo2curves 0.2.1:
 * x.c0 || x.c1 little-endian, bit 7 of byte 63 = parity of y.c0, identity = zeros.  Host arithmetic; ctx may be NULL. */
int h2agg_g2_batch_decompress(h2agg_ctx* ctx, const uint8_t* in, size_t n, uint8_t* out_aff);
int h2agg_pairing_product(h2agg_ctx* ctx, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, uint8_t out_gt[384]);
int h2agg_final_pair_check(h2agg_ctx* ctx, const uint8_t left_aff[64], const uint8_t right_aff[64],
                           const uint8_t s_g2[128], const uint8_t g2[128], int* ok);

/* ---- KZG parameters (what the reference's workflow does before verify_run: ParamsKZG::setup / downsize) ----------
 * halo2_proofs is an unvendored git dependency of the reference: the functions named below are recalled from upstream
 * (DESIGN.md section 2); what the entry points compute is the definition written next to each.
 *
 * h2agg_bases_fft — stands for: g_to_lagrange / ParamsKZG::downsize (inverse != 0) and the G1 best_fft it runs (inverse == 0).
 *   out[i] = sum_j w^(i*j) * in[j]                 (inverse == 0)
 *   out[i] = (1/n) * sum_j w^(-i*j) * in[j]        (inverse != 0; this is g_to_lagrange)
 *   n = 2^k, w = FR_ROOT_OF_UNITY^(2^(28-k)) (EvaluationDomain::get_omega).
 *   Reads the FIRST 2^k points of the table (a longer table is "downsized"); the table is not modified.  The result is a new
 *   resident base table of 2^k canonical affine points (identity = (0,0)), like any other: h2agg_bases_download / _free /
 *   _precompute, the MSM entry points and h2agg_instance_commitment accept it.
 *   k > 24, or 2^k longer than the input table: H2AGG_ERR_INVALID.  Out of memory: H2AGG_ERR_NOMEM, nothing is registered. */
int h2agg_bases_fft(h2agg_ctx* ctx, uint64_t in_handle, unsigned k, int inverse, uint64_t* out_handle);

/* stands for: ParamsKZG::setup with the trapdoor given by the caller (unsafe_setup / setup(k, rng) draw it themselves):
 *   g[i] = s^i * G,   g_lagrange[i] = L_i(s) * G with L_i(s) = w^i * (s^n - 1) / (n * (s - w^i)),   i < n = 2^k.
 * Either handle pointer may be NULL (that table is not built).  s: 32-byte little-endian, canonical (>= r:
 * H2AGG_ERR_NONCANONICAL).  k > 24: H2AGG_ERR_INVALID.
 * Two deviations from halo2_proofs, both H2AGG_ERR_INVALID here: s^n == 1 (there `(s - w^i).invert().unwrap()` panics), and
 * s == 0 (there every g[i] with i > 0 is the identity and the parameters are useless). */
int h2agg_params_setup(h2agg_ctx* ctx, unsigned k, const uint8_t s[32], uint64_t* g_handle_out, uint64_t* g_lagrange_handle_out);

/* Host-only, no context (like h2agg_hash_digest_host): what a params file needs beside the G1 tables.
 * h2agg_g2_scalar_mul — stands for: `s_g2 = g2 * s` of ParamsKZG::setup.  128-byte affine in and out (the form of
 *   h2agg_final_pair_check); the point must be canonical, on the twist and in the order-r subgroup, s canonical.
 * h2agg_g2_batch_compress — stands for: G2Affine::to_bytes as ParamsKZG::write uses it; the inverse of
 *   h2agg_g2_batch_decompress (128-byte affine -> 64 bytes: x.c0 || x.c1, bit 7 of byte 63 = parity of y.c0, identity = zeros). */
int h2agg_g2_scalar_mul(const uint8_t g2_aff[128], const uint8_t s[32], uint8_t out_aff[128]);
int h2agg_g2_batch_compress(const uint8_t* aff, size_t n, uint8_t* out);

/* ---- Fourier transform over Fr (the other primitive of halo2_proofs' create_proof beside best_multiexp) -------------
 * h2agg_fr_fft — stands for: best_fft and EvaluationDomain::{lagrange_to_coeff, coeff_to_lagrange, coeff_to_extended,
 * extended_to_coeff}.  halo2_proofs is an unvendored git dependency of the reference: these are recalled from upstream, not
 * pinned; what the entry points compute is this definition.  n = 2^k, w = FR_ROOT_OF_UNITY^(2^(28-k))
 * (the w of h2agg_bases_fft), natural order in and out:
 *   out[i] = sum_j (shift^j * in[j]) * w^(i*j)                  (inverse == 0)
 *   out[j] = shift^(-j) * (1/n) * sum_i in[i] * w^(-i*j)        (inverse != 0)
 * shift == NULL means 1: the plain best_fft / ifft.  shift = ZETA (the cube root of unity that is also the GLV eigenvalue)
 * gives coeff_to_extended / extended_to_coeff on input already padded to the extended size; any non-zero canonical shift is
 * accepted, and the inverse with a shift undoes the forward transform with the same shift exactly.
 * Elements are 32-byte canonical little-endian.  k == 0 copies the element (shift^0 = 1).
 * k > 24: H2AGG_ERR_INVALID (larger domains are out of scope: the passes index with 32 bits and the work array is one
 * allocation).  shift >= r: H2AGG_ERR_NONCANONICAL.  shift == 0: H2AGG_ERR_INVALID.  Out of memory: H2AGG_ERR_NOMEM.  The
 * context stays usable after any of them.
 * h2agg_fr_fft: host buffers, pageable or from h2agg_host_alloc; out == in is allowed; synchronous.  An element >= r:
 *   H2AGG_ERR_NONCANONICAL from the call; `out` is then unspecified.
 * h2agg_fr_fft_device: 2^k elements in DEVICE memory in and out, d_out == d_in allowed (otherwise the two must not overlap);
 *   queued on the context's stream, no synchronisation (a workspace that has to grow for a larger k than any before drains
 *   the device first).  The buffer rules of h2agg_set_stream / h2agg_g1_msm_device_async hold: d_in complete on that stream
 *   before the call, neither buffer touched until the stream has passed the transform.  An element >= r raises the
 *   context's device status: H2AGG_ERR_NONCANONICAL at h2agg_synchronize or at the next synchronous entry point, once; d_out
 *   is then unspecified. */
int h2agg_fr_fft(h2agg_ctx* ctx, const uint8_t* in, unsigned k, int inverse, const uint8_t shift[32], uint8_t* out);
int h2agg_fr_fft_device(h2agg_ctx* ctx, const void* d_in, unsigned k, int inverse, const uint8_t shift[32], void* d_out);

/* h2agg_fr_fft_batch — the transform above over a slab: `in` and `out` are host slabs [m][2^k] (pageable or from
 * h2agg_host_alloc), column j at byte 32 * 2^k * j; out == in is allowed; synchronous.  Column j of `out` is byte for byte
 * what h2agg_fr_fft returns for column j of `in` with the same k, inverse and shift.  All columns of a call share one shift
 * table and every pass of the transform is one launch over all of them (in chunks of as many columns as the context's work
 * array holds: DESIGN.md 5.8), which is what makes many small columns cheaper than as many calls.  This is what a prover does
 * to all its Lagrange columns at once (lagrange_to_coeff of every advice column) and what h2agg_quotient does inside.
 * Refusals: those of h2agg_fr_fft, and m == 0: H2AGG_ERR_INVALID.  The slab is staged whole (as h2agg_fr_poly_eval stages its
 * slab): one the device cannot hold is H2AGG_ERR_NOMEM.  An element >= r in any column: H2AGG_ERR_NONCANONICAL from the call;
 * `out` is then unspecified.  The context stays usable after any of them.  The resident form is h2agg_columns_fft. */
int h2agg_fr_fft_batch(h2agg_ctx* ctx, const uint8_t* in, size_t m, unsigned k, int inverse, const uint8_t shift[32],
                       uint8_t* out);

/* ---- KZG openings: evaluation, division by (X - z), the GWC multiopen prover -------------------------------------------
 * Stand for: eval_polynomial and kate_division (halo2_proofs arithmetic.rs) and the prover of poly/kzg/multiopen/gwc
 * (prover.rs).  halo2_proofs is an unvendored git dependency of the reference: recalled from upstream, not pinned (DESIGN.md
 * section 2); what the entry points compute is this definition.  Which W a verifier accepts IS pinned:
 * halo2-snark-aggregator-api/src/systems/halo2/multiopen.rs:23-69 (one W per distinct point in first-seen order, the queries of
 * a point folded with v^0 for the first), the verifier half being h2agg_schema_batch_multi_open above.
 *
 * A polynomial is n = 2^k canonical 32-byte little-endian Fr coefficients a[0..n), low degree first, k <= 24.
 *   eval      a(z) = sum_i a[i] z^i
 *   divide    q[j] = sum_{i>j} a[i] z^(i-j-1) for j < n, so q[n-1] = 0;  rem = a(z).  Then a(X) = q(X) (X - z) + rem.
 *             q is written as n elements with the zero on top, so it goes straight into an MSM over 2^k bases (halo2's
 *             kate_division returns the first n - 1).  q does not depend on a[0]: dividing a and dividing a - a(z) give the
 *             same quotient.
 *   multiopen npoly polynomials of one k, npoints points, nq queries, a challenge v.  A query is a pair of uint32_t
 *             {polynomial index, point index}; `queries` holds nq such pairs.  Queries are grouped by point index in
 *             first-seen order (multiopen.rs:31-43 with the point index in the rotation's role).  Group g with queries
 *             p_0, p_1, ... (in query order) at point z_g gives c_g(X) = sum_m v^m p_m(X) and
 *             W_g = sum_j quot(c_g, z_g)[j] * g[j] against the monomial table (ParamsKZG.g, e.g. from h2agg_params_setup).
 *             A polynomial may appear in several groups and more than once in one; points that no query names are ignored.
 * z == 0 (and v == 0) are legal everywhere.
 *
 * h2agg_fr_poly_eval / _device: `polys` is a slab [npoly][2^k] in host (pageable or h2agg_host_alloc) / DEVICE memory;
 *   queries and points (npoints x 32 bytes) are host memory; out = nq x 32 bytes to the host, out[q] = the value of query q;
 *   synchronous.  All queries go through one set of launches.
 * h2agg_fr_poly_divide: host buffers, out = 2^k elements, out == in allowed, rem = 32 bytes; synchronous.
 * h2agg_fr_poly_divide_device: 2^k elements in DEVICE memory in and out, d_quot == d_poly allowed (otherwise the two must not
 *   overlap); d_rem is 32 bytes of device memory or NULL; queued on the context's stream, no synchronisation.  The buffer
 *   rules are those of h2agg_fr_fft_device (complete on that stream before the call, untouched until the stream has passed
 *   the call; a workspace that has to grow drains the device first).
 * h2agg_kzg_multiopen_device / h2agg_kzg_multiopen: the slab in DEVICE / host memory; g_handle a resident base table of at
 *   least 2^k points.  Writes, to the host: *ngroups, one canonical affine W per group (64 bytes each, identity = zeros) to
 *   w_aff and each group's point index to group_points — both with room for min(nq, npoints) entries; synchronous.  The work
 *   memory is one quotient slab [groups][2^k] kept in the context (128 MiB per group at k = 22), committed by
 *   h2agg_g1_msm_device_batch_async.  With the debug key "phases", h2agg_last_phases gives the call's split.
 * Refusals, the context stays usable after each: k > 24, a null buffer, nq == 0 or nq > 65535, a polynomial index >= npoly,
 *   a point index >= npoints, a table shorter than 2^k or an unknown handle: H2AGG_ERR_INVALID.  A point, z or v >= r:
 *   H2AGG_ERR_NONCANONICAL.  A coefficient >= r: H2AGG_ERR_NONCANONICAL through the context's device status — from the call for
 *   the synchronous entry points, at h2agg_synchronize (or the next synchronous entry point), once, for
 *   h2agg_fr_poly_divide_device; outputs are then unspecified.  Out of memory: H2AGG_ERR_NOMEM. */
int h2agg_fr_poly_eval(h2agg_ctx* ctx, const uint8_t* polys, size_t npoly, unsigned k, const uint32_t* queries, size_t nq,
                       const uint8_t* points, size_t npoints, uint8_t* out);
int h2agg_fr_poly_eval_device(h2agg_ctx* ctx, const void* d_polys, size_t npoly, unsigned k, const uint32_t* queries, size_t nq,
                              const uint8_t* points, size_t npoints, uint8_t* out);
int h2agg_fr_poly_divide(h2agg_ctx* ctx, const uint8_t* in, unsigned k, const uint8_t z[32], uint8_t* out, uint8_t rem[32]);
int h2agg_fr_poly_divide_device(h2agg_ctx* ctx, const void* d_poly, unsigned k, const uint8_t z[32], void* d_quot, void* d_rem);
int h2agg_kzg_multiopen(h2agg_ctx* ctx, uint64_t g_handle, const uint8_t* polys, size_t npoly, unsigned k, const uint32_t* queries,
                        size_t nq, const uint8_t* points, size_t npoints, const uint8_t v[32], uint8_t* w_aff,
                        uint32_t* group_points, size_t* ngroups);
int h2agg_kzg_multiopen_device(h2agg_ctx* ctx, uint64_t g_handle, const void* d_polys, size_t npoly, unsigned k,
                               const uint32_t* queries, size_t nq, const uint8_t* points, size_t npoints, const uint8_t v[32],
                               uint8_t* w_aff, uint32_t* group_points, size_t* ngroups);

/* ---- KZG openings, Shplonk: the BDFG20 multiopen prover -------------------------------------------------------------------
 * Stand for: the prover of poly/kzg/multiopen/shplonk (prover.rs) and construct_intermediate_sets of halo2_proofs — an
 * unvendored git dependency of the reference: recalled from upstream, not pinned; what the entry points
 * compute is this definition, and what is pinned is its algebra and the verifier equation at its end.
 *
 * Inputs as for h2agg_kzg_multiopen: npoly polynomials of one k <= 24 as a slab [npoly][2^k] in host memory, npoints points, nq
 * queries {polynomial index, point index}; and evals, nq x 32 bytes, the value of each query as the caller wrote it to its
 * transcript; challenges y and v, and later u.
 *   Sets.   A polynomial's point set is the set of point indices its queries name (a repeated pair counts once).  Polynomials
 *           with equal point sets form set i; sets are numbered in first-seen order of their first polynomial, the polynomials
 *           p_{i,0}, p_{i,1}, ... inside a set in first-seen order of their first query.  S_i: the set's points; T: the union of
 *           all named points.  (halo2's own ordering of the sets belongs to construct_intermediate_sets: a caller that needs
 *           it orders its queries accordingly.)  Points and polynomials that no query names are ignored.
 *   Round 1 r_{i,j}: the polynomial of degree < |S_i| with r_{i,j}(z) = evals at z in S_i (interpolated on the host).
 *             N_i(X) = sum_j y^j (p_{i,j}(X) - r_{i,j}(X))
 *             h(X)   = sum_i v^i N_i(X) / Z_{S_i}(X),      Z_S(X) = prod_{z in S} (X - z)
 *             H1     = sum_j h[j] g[j]
 *           Powers ascend, the first term at power 0 (as in the GWC definition above).
 *   Round 2 With d_i = Z_{T \ S_i}(u), c_i = d_i / d_0 and t = Z_T(u) / d_0:
 *             L(X)  = sum_i v^i c_i sum_j y^j (p_{i,j}(X) - r_{i,j}(u))  -  t h(X)
 *             h2(X) = L(X) / (X - u),      H2 = sum_j h2[j] g[j]
 *   Verifier equation, C_{i,j} the commitment of p_{i,j} and G = g[0]:
 *             F = sum_i v^i c_i sum_j y^j (C_{i,j} - r_{i,j}(u) G) - t H1;   left = H2;   right = F + u H2
 *           accepted iff e(left, s_g2) e(right, -g2) = 1: what h2agg_final_pair_check takes.
 * y, v, u and points equal to 0 are legal, and so is u in S_0.  A zero h or h2 gives the identity, 64 zero bytes.
 *
 * h2agg_kzg_shplonk_begin: stages the slab once, runs round 1, writes H1 (canonical affine) to h1_aff and the object to *out;
 *   synchronous.  The object keeps, in device memory, the slab with h behind it ((npoly + 1) 2^k elements) and one more array of
 *   2^k; it refers to ctx and g_handle, which must outlive it, and is used from the context's thread.
 * h2agg_kzg_shplonk_finish: runs round 2 for u, writes H2 to h2_aff; synchronous; may be called again with another u.
 * h2agg_kzg_shplonk_destroy: frees the object (NULL: nothing).
 * With the debug key phases, h2agg_last_phases gives " stage=ms numerators=ms divide=ms commit=ms" after begin and
 * " combine=ms divide=ms commit=ms" after finish, from events on the context's stream.  The key fr_poly_chunk is honoured.
 * Refusals, the context stays usable after each and begin leaves no object (*out = NULL): those of h2agg_kzg_multiopen (k > 24,
 *   a null buffer, nq == 0 or nq > 65535, an index out of range, a table shorter than 2^k or an unknown handle:
 *   H2AGG_ERR_INVALID; a point, a value, y, v or u >= r: H2AGG_ERR_NONCANONICAL; a coefficient >= r of a polynomial some query
 *   names: H2AGG_ERR_NONCANONICAL through the context's device status, from the call; out of memory: H2AGG_ERR_NOMEM), and, all
 *   H2AGG_ERR_INVALID: a repeated (polynomial, point) pair with two different values; two named point indices holding equal
 *   values; a set of more than 32 points; some N_i(z) != 0 for a z in S_i, i.e. a value that is not its polynomial's (the
 *   message names the query); in finish, d_0 == 0: u is a point of T \ S_0.  A non-zero remainder L(u), which values that
 *   begin accepted cannot give: H2AGG_ERR_HIP (the library's code for a failure of the device). */
typedef struct h2agg_shplonk h2agg_shplonk;
int h2agg_kzg_shplonk_begin(h2agg_ctx* ctx, uint64_t g_handle, const uint8_t* polys, size_t npoly, unsigned k, const uint32_t* queries,
                            size_t nq, const uint8_t* points, size_t npoints, const uint8_t* evals, const uint8_t y[32],
                            const uint8_t v[32], uint8_t h1_aff[64], h2agg_shplonk** out);
int h2agg_kzg_shplonk_finish(h2agg_shplonk* obj, const uint8_t u[32], uint8_t h2_aff[64]);
void h2agg_kzg_shplonk_destroy(h2agg_shplonk* obj);

/* ---- Grand products: batch inversion, the permutation and lookup Z columns ------------------------------------------------
 * Stand for: ff::BatchInvert, permutation::prover::commit and lookup::prover::commit_product of halo2_proofs — an unvendored
 * git dependency of the reference: recalled from upstream, not pinned; what the entry points compute
 * is this definition.  Which Z a verifier accepts IS pinned: halo2-snark-aggregator-api/src/systems/halo2/permutation.rs:70-133
 * (l_0 (1 - z_0); l_last (z^2 - z) on the last set; l_0 (z_i - z_{i-1}(w^last X)) between sets; the row identity
 * z(wX) prod(p + beta s + gamma) = z(X) prod(p + delta^j beta X + gamma)) and lookup.rs:98-113
 * (z(wX)(a' + beta)(s' + gamma) = z(X)(a + beta)(s + gamma)).
 *
 * All elements are canonical 32-byte little-endian Fr.  Row i of a column of n = 2^k rows sits at w^i, w the root
 * h2agg_fr_fft uses for k, k <= 24.  u is the number of usable rows (n - (blinding_factors + 1) in halo2), 0 <= u <= n - 1.
 *   batch_invert         out[i] = in[i]^-1, and out[i] = 0 where in[i] = 0 (ff::BatchInvert: zeros are skipped, a zero is not
 *                        an error — h2agg_fr_batch_op(INV) answers H2AGG_ERR_DIV_ZERO).  Any 0 <= n <= 2^24, not only powers
 *                        of two; n == 0 is a no-op.
 *   grand_product        out[0] = init, out[i+1] = out[i] * num[i] * inv(den[i]) for i < u, with inv(0) = 0 as above.  den may
 *                        be NULL: a plain running product.  num and den have at least u elements; exactly u + 1 elements of
 *                        out are written (in halo2 the rows above u belong to the caller's blinding).  last[32] is optional
 *                        and receives out[u].
 *   permutation_product  one permutation set of m columns, 1 <= m <= 16; values and sigmas are slabs [m][n] in Lagrange form.
 *                          num[i] = prod_j (values[j][i] + beta * dj * w^i + gamma),  dj = delta_first * delta^j
 *                          den[i] = prod_j (values[j][i] + beta * sigmas[j][i] + gamma)
 *                        The result is grand_product(num, den, u, init).  delta, delta_first (delta^(set_index * chunk_len))
 *                        and init (the previous set's z[u], or 1) are arguments: the library holds no literal for them.
 *   lookup_product       compressed input a, compressed table s, their permuted forms ap and sp, n rows each.
 *                          num[i] = (a[i] + beta)(s[i] + gamma),  den[i] = (ap[i] + beta)(sp[i] + gamma)
 *                        The result is grand_product(num, den, u, 1).  The theta-compression of the expressions (a linear
 *                        combination) and permute_expression_pair (a sort) are the caller's job.  Both are entry points of
 *                        the next block: h2agg_fr_columns_compress and h2agg_lookup_permute.
 * Only rows i < u of a column are read.
 *
 * Every entry point is synchronous over host buffers (pageable or h2agg_host_alloc) and has a _device twin over DEVICE
 * memory that is queued on the context's stream with no synchronisation; the buffer rules are those of h2agg_fr_fft_device
 * (inputs complete on that stream before the call, nothing touched until the stream has passed the call; a workspace that
 * has to grow drains the device first).  Outputs must not overlap inputs, except: d_out == d_in for batch_invert (and
 * out == in for the host form), and d_out may alias d_num for grand_product.  d_last is 32 bytes of device memory or NULL.
 * The work memory — the num and den columns and the chunk products — is kept in the context.
 * Refusals, the context stays usable after each: k > 24, n > 2^24, u >= 2^k, m == 0 or m > 16, a null required buffer:
 *   H2AGG_ERR_INVALID.  beta, gamma, delta, delta_first or init >= r: H2AGG_ERR_NONCANONICAL from the call.  A column element
 *   >= r: H2AGG_ERR_NONCANONICAL through the context's device status — from the call for the synchronous entry points, at
 *   h2agg_synchronize (or the next synchronous entry point), once, for the _device twins; outputs are then unspecified.  Out
 *   of memory: H2AGG_ERR_NOMEM. */
int h2agg_fr_batch_invert(h2agg_ctx* ctx, const uint8_t* in, size_t n, uint8_t* out);
int h2agg_fr_batch_invert_device(h2agg_ctx* ctx, const void* d_in, size_t n, void* d_out);
int h2agg_fr_grand_product(h2agg_ctx* ctx, const uint8_t* num, const uint8_t* den, unsigned k, size_t u, const uint8_t init[32],
                           uint8_t* out, uint8_t last[32]);
int h2agg_fr_grand_product_device(h2agg_ctx* ctx, const void* d_num, const void* d_den, unsigned k, size_t u, const uint8_t init[32],
                                  void* d_out, void* d_last);
int h2agg_permutation_product(h2agg_ctx* ctx, const uint8_t* values, const uint8_t* sigmas, size_t m, unsigned k, size_t u,
                              const uint8_t beta[32], const uint8_t gamma[32], const uint8_t delta[32],
                              const uint8_t delta_first[32], const uint8_t init[32], uint8_t* out, uint8_t last[32]);
int h2agg_permutation_product_device(h2agg_ctx* ctx, const void* d_values, const void* d_sigmas, size_t m, unsigned k, size_t u,
                                     const uint8_t beta[32], const uint8_t gamma[32], const uint8_t delta[32],
                                     const uint8_t delta_first[32], const uint8_t init[32], void* d_out, void* d_last);
int h2agg_lookup_product(h2agg_ctx* ctx, const uint8_t* a, const uint8_t* s, const uint8_t* ap, const uint8_t* sp, unsigned k,
                         size_t u, const uint8_t beta[32], const uint8_t gamma[32], uint8_t* out, uint8_t last[32]);
int h2agg_lookup_product_device(h2agg_ctx* ctx, const void* d_a, const void* d_s, const void* d_ap, const void* d_sp, unsigned k,
                                size_t u, const uint8_t beta[32], const uint8_t gamma[32], void* d_out, void* d_last);

/* ---- Lookup argument: theta-compression and permute_expression_pair ---------------------------------------------------------
 * Stand for: the theta-fold of lookup::prover::commit_permuted and lookup::prover::permute_expression_pair of halo2_proofs —
 * recalled from upstream, not pinned, like the block above; what the entry points compute is this definition.  Which pair a
 * verifier accepts IS pinned (lookup.rs:98-113): on the rows below u, ap[0] = sp[0]; every row has ap[i] = sp[i] or
 * ap[i] = ap[i-1]; ap is a permutation of a and sp one of s (which is what makes z[u] = 1).
 *
 * Elements, columns (n = 2^k rows, k <= 24) and u (0 <= u <= n - 1) are those of the block above.
 *   lookup_permute(a, s, k, u) -> ap[0..u), sp[0..u)
 *     - ap[0..u) is a[0..u) in ascending order of the canonical integer value (halo2curves' Ord for Fr).
 *     - Row i is a head if i == 0 or ap[i] != ap[i-1].  For a head sp[i] = ap[i], and one occurrence of that value is taken
 *       out of the multiset s[0..u).
 *     - What is left of the multiset, in ascending order and with repeats kept, fills the non-head rows from the highest row
 *       down: the j-th leftover value goes to the j-th non-head row counted from row u - 1 (halo2's
 *       repeated_input_rows.pop() over an ascending BTreeMap).
 *     - Rows from u up of a and s are not read; rows from u up of ap and sp are not written (the caller's blinding rows).
 *     - A head value that does not occur in s[0..u): H2AGG_ERR_NOT_IN_TABLE (halo2: Error::ConstraintSystemFailure); the
 *       outputs are then unspecified.  u == 0 writes nothing and succeeds.
 *   columns_compress(cols[m][n], theta) -> out[n]:  out[i] = sum_j theta^(m-1-j) cols[j][i] — halo2's fold
 *       acc * theta + expr, the first expression under the highest power; 1 <= m <= 65536, all n rows.
 *
 * The plain entry points are synchronous over host buffers; the _device twins are queued on the context's stream with no
 * synchronisation and no host read-back between their kernels (buffer rules: h2agg_fr_fft_device; a workspace that has to
 * grow drains the device first).  d_ap and d_sp must not overlap d_a, d_s or each other; d_out of the compression may be
 * one of its columns.  The work memory of lookup_permute — four key buffers, five 32-bit columns and the count matrix of a
 * sort pass, about 150 bytes per row — is kept in the context.
 * Refusals, the context stays usable after each: k > 24, u >= 2^k, m == 0 or m > 65536, a null buffer, overlapping device
 *   ranges: H2AGG_ERR_INVALID.  theta >= r: H2AGG_ERR_NONCANONICAL from the call.  A column element >= r
 *   (H2AGG_ERR_NONCANONICAL) or an absent head value (H2AGG_ERR_NOT_IN_TABLE): through the context's device status — from the
 *   call for the synchronous entry points, at h2agg_synchronize (or the next synchronous entry point), once, for the _device
 *   twins.  Out of memory: H2AGG_ERR_NOMEM. */
int h2agg_lookup_permute(h2agg_ctx* ctx, const uint8_t* a, const uint8_t* s, unsigned k, size_t u, uint8_t* ap, uint8_t* sp);
int h2agg_lookup_permute_device(h2agg_ctx* ctx, const void* d_a, const void* d_s, unsigned k, size_t u, void* d_ap, void* d_sp);
int h2agg_fr_columns_compress(h2agg_ctx* ctx, const uint8_t* cols, size_t m, unsigned k, const uint8_t theta[32], uint8_t* out);
int h2agg_fr_columns_compress_device(h2agg_ctx* ctx, const void* d_cols, size_t m, unsigned k, const uint8_t theta[32], void* d_out);

/* ---- Lookup argument, batched: every lookup of a circuit in one call ---------------------------------------------------------
 * Lookup j of a batch of `count` is EXACTLY h2agg_lookup_permute / h2agg_lookup_product (the two blocks above) on column j of
 * each slab, byte for byte; what a batch changes is the number of launches: all lookups of a chunk share the launches of one
 * (DESIGN.md 5.21).  Slabs are [count][2^k] (column j at 32 * 2^k * j bytes); u, beta, gamma are the batch's.
 *   lookup_batch_permute(a, s, count, k, u) -> ap, sp, status[count]
 *   lookup_batch_product(a, s, ap, sp, count, k, u, beta, gamma) -> z, last[count][32]
 *   lookup_store_permute / lookup_store_product: the same over column stores (the block "Fr column stores" below): columns
 *     first .. first + count - 1 of each named store, k the stores'.  The stores may be one store with disjoint ranges.
 *     - Rows from u up of ap and sp, rows from u + 1 up of z are not written (the caller's blinding rows); columns of a store
 *       outside the named ranges are not touched.  u == 0: z[j][0] = 1 and nothing else is written.
 *     - status[j] (may be NULL) is 0, or the OR of the status bits of lookup j: H2AGG_LOOKUP_STATUS_NONCANONICAL (1) = an
 *       element >= r, H2AGG_LOOKUP_STATUS_NOT_IN_TABLE (8) = a head value absent from its table.  last[j] (may be NULL) =
 *       z[j][u].
 *     - The host-slab forms are synchronous.  A store form that is given status (permute) or last (product) is synchronous
 *       too.  A synchronous call returns the code the single call would return for the LOWEST-NUMBERED failing lookup
 *       (H2AGG_ERR_NONCANONICAL, H2AGG_ERR_NOT_IN_TABLE); the outputs of every lookup that did not fail are complete and
 *       correct, those of a failed one unspecified.
 *     - A store form with status == NULL / last == NULL is queued on the context's stream with no synchronisation and no
 *       read-back, and reports through the context's device status as the _device twins above do (a workspace that has to
 *       grow drains the device first).
 *   lookup_configure(batch_chunk): at most that many lookups per chunk (set of launches) in this context; 0 = the default,
 *     clamp(2^24 / max(u, 1), 1, 1024).  lookup_chunk_rule(u, batch_chunk) -> the lookups per chunk a context configured
 *     with batch_chunk takes at u rows (host arithmetic, no context; a batch_chunk above 1024 counts as 0).  Work memory per chunk of B lookups: B times a single call's (about 150 bytes per row),
 *     kept in the context.
 * Refusals, the context stays usable and nothing is written: those of the single calls (k > 24, u >= 2^k, a null buffer,
 *   beta / gamma >= r: H2AGG_ERR_NONCANONICAL) and of the store family (an unknown handle, a range outside its store, stores
 *   that differ in k); count == 0 or count > 65535; an output range that overlaps an input range or another output;
 *   batch_chunk > 1024: H2AGG_ERR_INVALID.  Out of memory: H2AGG_ERR_NOMEM.
 * Debug key phases: h2agg_last_phases gives " sort= rank=" (permute) and " terms= invert= scan=" (product), milliseconds on
 *   the context's stream; the host-slab forms put " stage=" in front. */
#define H2AGG_LOOKUP_STATUS_NONCANONICAL 1u
#define H2AGG_LOOKUP_STATUS_NOT_IN_TABLE 8u
int h2agg_lookup_batch_permute(h2agg_ctx* ctx, const uint8_t* a, const uint8_t* s, size_t count, unsigned k, size_t u,
                               uint8_t* ap, uint8_t* sp, uint32_t* status);
int h2agg_lookup_batch_product(h2agg_ctx* ctx, const uint8_t* a, const uint8_t* s, const uint8_t* ap, const uint8_t* sp,
                               size_t count, unsigned k, size_t u, const uint8_t beta[32], const uint8_t gamma[32],
                               uint8_t* z, uint8_t* last);
int h2agg_lookup_store_permute(h2agg_ctx* ctx, uint64_t a, size_t afirst, uint64_t s, size_t sfirst, size_t count, size_t u,
                               uint64_t ap, size_t apfirst, uint64_t sp, size_t spfirst, uint32_t* status);
int h2agg_lookup_store_product(h2agg_ctx* ctx, uint64_t a, size_t afirst, uint64_t s, size_t sfirst, uint64_t ap, size_t apfirst,
                               uint64_t sp, size_t spfirst, size_t count, size_t u, const uint8_t beta[32],
                               const uint8_t gamma[32], uint64_t z, size_t zfirst, uint8_t* last);
int h2agg_lookup_configure(h2agg_ctx* ctx, size_t batch_chunk);
size_t h2agg_lookup_chunk_rule(size_t u, size_t batch_chunk);

/* ---- Quotient polynomial h(X): a key's expressions on every row, and the quotient from the verifying key ---------------------
 * Stand for: the evaluation of h(X) in halo2_proofs' create_proof (evaluate_h, coeff_to_extended, extended_to_coeff) — recalled
 * from upstream, not pinned, like the blocks above; what the entry points compute is this definition.  Which expressions h
 * has to satisfy, and in which order, IS pinned: halo2-snark-aggregator-api/src/systems/halo2/params.rs:74-224 (gates, then the
 * permutation argument, then every lookup), permutation.rs:54-136, lookup.rs:34-119, and vanish.rs:18-72 for how the verifier
 * puts the pieces of h together.
 *
 * Elements are canonical 32-byte little-endian Fr; n = 2^k is the key's; columns are slabs [columns][n]:
 * advice[num_advice_columns][n], fixed[nfixed][n] (nfixed = the key's number of fixed commitments), instance[
 * num_instance_columns][n]; challenges = num_challenges x 32 bytes.  A slab whose count is zero may be NULL.
 *
 * h2agg_vk_expressions_eval — expressions of the key on every row i < n of value slabs.
 *   which = 0: every gate polynomial in key order (gate by gate, poly by poly); 1: the input expressions of lookup j;
 *   2: the table expressions of lookup j (j is ignored for which = 0).  The list has m expressions E_0 .. E_{m-1}.
 *   Leaves: FIXED / ADVICE / INSTANCE(q) reads column queries[q].column of its slab at row (i + queries[q].rotation) mod n —
 *   the mathematical modulus: negative rotations and |rotation| >= n are legal; CHALLENGE(c) and CONST are scalars; NEG, SUM,
 *   PRODUCT, SCALED are the field operations.
 *   fold == NULL: out is [m][n], out[j][i] = E_j(row i).  fold = 32 bytes: out is [n], out[i] = sum_j fold^(m-1-j) E_j(row i)
 *   (acc * fold + E, the first expression under the highest power): fold = theta on a lookup's lists gives the two compressed
 *   columns commit_permuted sorts, fold = y on the gates the gates' share of the quotient's numerator.
 *   The operand stack of an expression (values alive at once while its postfix form runs) may be H2AGG_EXPR_MAX_DEPTH deep;
 *   a deeper expression is H2AGG_ERR_INVALID from this call (h2agg_vk_create accepts what it always did).
 *
 * h2agg_quotient — the pieces of h from polynomials in COEFFICIENT form, n coefficients each, low degree first:
 *   advice, fixed, instance as above; sigma[P][n] (P = the key's permutation columns), perm_z[n_sets][n] (n_sets =
 *   ceil(P / chunk_len), chunk_len = degree - 2), lookup_z, lookup_ap, lookup_sp [L][n] each (L = the key's lookups); the
 *   scalars challenges, theta, beta, gamma, y and delta (as in h2agg_permutation_product the library holds no literal for
 *   delta).  Output h[degree - 1][n]: the pieces h_0 .. h_{degree-2}.
 *   Let bf = blinding_factors, u = n - bf - 1; w the root h2agg_fr_fft uses for k; l_i the Lagrange polynomial of row i over
 *   {w^i}; l_last = l_u, l_blind = l_{u+1} + .. + l_{n-1}, act = 1 - l_last - l_blind; c = chunk_len; a column polynomial p
 *   at rotation t is p(w^t X).  The list E_0 .. E_{m-1}, as polynomial identities in X:
 *     gates        every gate polynomial, leaves as above;
 *     permutation  (only if n_sets > 0)  l_0 (1 - z_0);  l_last (z_last^2 - z_last), z_last the last set's;
 *                  for i = 1 .. n_sets-1: l_0 (z_i - z_{i-1}(w^u X))   (w^u = w^-(bf+1): the "last" rotation);
 *                  for every set s over its columns j, g = s c + j, v_g the polynomial of permutation column g:
 *                  act ( z_s(wX) prod_j (v_g + beta sigma_g + gamma) - z_s(X) prod_j (v_g + delta^g beta X + gamma) );
 *     per lookup   with A, S the theta-folds of its input / table expressions:  l_0 (1 - z);  l_last (z^2 - z);
 *                  act ( z(wX)(a' + beta)(s' + gamma) - z(X)(A + beta)(S + gamma) );  l_0 (a' - s');
 *                  act (a' - s')(a' - a'(w^-1 X)).
 *   N = sum_i y^(m-1-i) E_i.  e = the smallest integer with 2^(k+e) >= n (degree - 1); w_ext = the root of h2agg_fr_fft for
 *   k + e (w_ext^(2^e) = w); zeta = the cube root of unity of coeff_to_extended (the `shift = ZETA` of h2agg_fr_fft).
 *   H = the unique polynomial of degree < 2^(k+e) with H(s) = N(s) / (s^n - 1) at every s = zeta w_ext^j, j < 2^(k+e);
 *   h_i = the coefficients [i n, (i+1) n) of H, i < degree - 1 (higher ones are dropped, as extended_to_coeff truncates).
 *   For a satisfied circuit H = N / (X^n - 1) exactly; for any other input it is still this one answer.
 *   Two routes give this one H, byte for byte.  k + e <= 24: the cosets' values are interleaved and one
 *   inverse transform of size 2^(k+e) ends the call.  24 < k + e <= 28 (28 is the two-adicity of Fr), k <= 24: the coset-split
 *   ending — every coset's fold goes through an inverse transform of size n at its own shift, and one kernel across the
 *   cosets turns the 2^e results of a row into its degree - 1 piece values; nothing larger than 2^k is transformed.
 *   The larger keys are h2agg_quotient_device's: the host-buffer form stages every slab whole and keeps k + e <= 24.
 *
 * h2agg_quotient_configure — split = 1: every h2agg_quotient* call of the context takes the coset-split ending, at every size
 *   (tests and A/B measurements below 2^24; the pieces are the same bytes on either route); split = 0, the default: by the
 *   rule above.  Any other value: H2AGG_ERR_INVALID, and the setting stays.
 *   Work memory, kept in the context: one coset's values of every polynomial, nine more columns and the
 *   extended evaluations (split route: the cosets' inverse transforms) — (the number of input polynomials + 9) n + 2^(k+e)
 *   elements, not columns x 2^(k+e) — and the transform's work array: max(W, min((the number of input polynomials + 3) n,
 *   2^23)) elements, W = 2^(k+e), on the split route n, so that a coset's transforms are one launch per pass
 *   (h2agg_fr_fft_batch's rule) wherever that fits 256 MiB.
 *
 * h2agg_quotient_work_bytes — that work memory in bytes for this key, 32 x (the two sums above) on the route the key takes by
 *   the rule above (h2agg_quotient_configure is a context's and is not seen here): what an h2agg_quotient* call will hold in the context beside the caller's columns (at k = 24 with 34
 *   input polynomials and e = 3: 51 + 1 columns of 512 MiB, 26 GiB).  Not counted: the compiled programs and the power tables
 *   (under 1 MiB together), the staging buffers of the host form, and the slack of the context's grow-only buffers, which
 *   allocate one eighth more than they are asked for.  Needs no context and no device.  A null argument, or a key that
 *   h2agg_quotient refuses by its shape (k > 24, k + e > 28): H2AGG_ERR_INVALID.
 *
 * The plain entry points are synchronous over host buffers (pageable or h2agg_host_alloc); the _device twins take DEVICE
 * memory and are queued on the context's stream with no synchronisation and no read-back (buffer rules: h2agg_fr_fft_device;
 * a workspace that has to grow drains the device first).  Outputs must not overlap inputs.  With the debug key "phases" a
 * quotient call waits for its own events and h2agg_last_phases gives " forward=ms gates=ms permutation=ms lookups=ms
 * inverse=ms".
 * Refusals, the context stays usable after each: an unknown `which` or j, k different from the key's (or > 24), a list
 * without expressions, a null required buffer, an expression deeper than H2AGG_EXPR_MAX_DEPTH; for the quotient also
 * k + e > 28 (h2agg_quotient: > 24), k > 24 and degree < 3 with permutation columns: H2AGG_ERR_INVALID.  A scalar (challenge, fold, theta, beta, gamma, y,
 * delta, a CONST of the key) >= r: H2AGG_ERR_NONCANONICAL from the call.  A column element >= r: H2AGG_ERR_NONCANONICAL through
 * the context's device status — from the call for the synchronous entry points, at h2agg_synchronize (or the next
 * synchronous entry point), once, for the _device twins; outputs are then unspecified.  Out of memory: H2AGG_ERR_NOMEM. */
#define H2AGG_EXPR_MAX_DEPTH 16
int h2agg_vk_expressions_eval(h2agg_ctx* ctx, const h2agg_vk* vk, int which, size_t j, unsigned k, const uint8_t* advice,
                              const uint8_t* fixed, const uint8_t* instance, const uint8_t* challenges, const uint8_t fold[32],
                              uint8_t* out);
int h2agg_vk_expressions_eval_device(h2agg_ctx* ctx, const h2agg_vk* vk, int which, size_t j, unsigned k, const void* d_advice,
                                     const void* d_fixed, const void* d_instance, const uint8_t* challenges, const uint8_t fold[32],
                                     void* d_out);
int h2agg_quotient(h2agg_ctx* ctx, const h2agg_vk* vk, const uint8_t* advice, const uint8_t* fixed, const uint8_t* instance,
                   const uint8_t* sigma, const uint8_t* perm_z, const uint8_t* lookup_z, const uint8_t* lookup_ap,
                   const uint8_t* lookup_sp, const uint8_t* challenges, const uint8_t theta[32], const uint8_t beta[32],
                   const uint8_t gamma[32], const uint8_t y[32], const uint8_t delta[32], uint8_t* h);
int h2agg_quotient_device(h2agg_ctx* ctx, const h2agg_vk* vk, const void* d_advice, const void* d_fixed, const void* d_instance,
                          const void* d_sigma, const void* d_perm_z, const void* d_lookup_z, const void* d_lookup_ap,
                          const void* d_lookup_sp, const uint8_t* challenges, const uint8_t theta[32], const uint8_t beta[32],
                          const uint8_t gamma[32], const uint8_t y[32], const uint8_t delta[32], void* d_h);
int h2agg_quotient_configure(h2agg_ctx* ctx, int split);
int h2agg_quotient_work_bytes(const h2agg_vk* vk, size_t* bytes_out);

/* ---- Keys: sigma columns from copy constraints, and the commitments of a slab of columns ------------------------------------
 * Stand for: permutation::keygen::Assembly (new, copy, build_vk, build_pk) and the commit_lagrange loops of keygen_vk /
 * keygen_pk of halo2_proofs — recalled from upstream, not pinned, like the blocks above; what the entry points compute is
 * this definition.  What a verifier does with the results IS pinned: the sigma commitments are the permutation commitments
 * of the H2VK blob (h2agg_vk_create), the sigma columns are the `sigmas` of h2agg_permutation_product and the `sigma` of
 * h2agg_quotient.
 *
 * Definitions.  A permutation over m columns of n = 2^k rows is a `mapping`: m * n pairs of uint32_t {column, row}, cell
 * (j, i) at index j * n + i (2 * m * n words).
 *   sigma[j][i] = delta^c * w^r  for {c, r} = mapping[j][i], w the 2^k-th root h2agg_fr_fft uses; delta is an argument
 *   (callers pass Fr::DELTA, as to h2agg_permutation_product: the library holds no literal for it).
 *   A mapping is valid when every entry has c < m and r < n, the entries are pairwise distinct (a bijection of the cells),
 *   and every cell with i >= usable maps to itself.
 *
 * h2agg_permutation_assembly — host arithmetic, no context (like h2agg_g2_scalar_mul).  copies holds ncopies quadruples
 *   {left column, left row, right column, right row}; the result is the mapping Assembly holds after copy() on them in order:
 *   mapping, aux (a cell's cycle representative) and sizes start as the identity, the cell itself and 1.  For a copy whose two
 *   cells have different representatives the representative of the smaller cycle is merged into the other one (on a tie the
 *   right cell's): the sizes add, the merged cycle is walked through mapping, rewriting aux, then mapping[left] and
 *   mapping[right] are swapped.  A copy within one cycle does nothing.  Cost O(m n + the sum of the merged sizes); work memory
 *   24 bytes per cell.  The result is a valid mapping whose cycles are the classes of the copies' equivalence relation.
 *   Refusals, H2AGG_ERR_INVALID with `mapping` untouched: k > 24, m == 0 or m > H2AGG_PERM_MAX_COLUMNS, usable > n, a null
 *   mapping, null copies with ncopies != 0, a column >= m, a row >= usable (keygen's assembly refuses unusable rows).
 *
 * h2agg_permutation_sigmas — host buffers, synchronous.  Writes the slab [m][n] of canonical 32-byte elements in Lagrange
 *   form to sigma_lagrange and the same columns in coefficient form (h2agg_fr_fft_batch's inverse transform, with its 1/n) to
 *   sigma_coeff.  Either output may be NULL, not both.  The mapping is checked: its range on the host in front of the copy,
 *   bijectivity (one bit per cell) and the identity rule on the device.
 *   Refusals: the limits above, a null mapping or delta, both outputs NULL, an invalid mapping: H2AGG_ERR_INVALID; delta >= r:
 *   H2AGG_ERR_NONCANONICAL.  On a refusal nothing is written to the outputs and the context stays usable.  Out of memory:
 *   H2AGG_ERR_NOMEM.  Work memory, kept in the context: the mapping, one or two slabs, m n / 8 bytes of bitmap.  With the
 *   debug key "phases" h2agg_last_phases gives " stage=ms sigma=ms inverse=ms copy=ms" (empty after a call the host refused,
 *   without copy= after one the device refused).
 *
 * h2agg_commit_columns — host buffers, synchronous.  columns is a slab [m][n] of canonical scalars; out_aff[64 j ..] =
 *   sum_i columns[j][i] * table[i] as a canonical affine point, the identity as 64 zero bytes (as in h2agg_kzg_multiopen).
 *   Against g_lagrange of h2agg_params_setup this is commit_lagrange of every column, against g it commits coefficient columns.
 *   The slab is staged once; the MSMs run through h2agg_g1_msm_device_batch_async in chunks of B columns per call, B =
 *   max(1, 2^22 / n) — the scalars in flight bound the sort's and the buckets' work memory — or the debug key "commit_chunk";
 *   that path cuts a chunk further by its own limits (its sort's counters and 32-bit offsets; one MSM at a time from 2^20
 *   points on).  Whatever the chunk, the points are the same bytes.
 *   Refusals: an unknown handle, a table shorter than n, m == 0, k > 24, a null buffer: H2AGG_ERR_INVALID.  A scalar >= r:
 *   H2AGG_ERR_NONCANONICAL through the context's device status, as h2agg_g1_msm_preloaded reports it; out_aff is then
 *   unspecified.  Out of memory: H2AGG_ERR_NOMEM.  The context stays usable after each.
 *
 * The resident forms are h2agg_columns_sigmas and h2agg_columns_commit, over column stores. */
#define H2AGG_PERM_MAX_COLUMNS 4096
int h2agg_permutation_assembly(size_t m, unsigned k, size_t usable, const uint32_t* copies, size_t ncopies, uint32_t* mapping);
int h2agg_permutation_sigmas(h2agg_ctx* ctx, const uint32_t* mapping, size_t m, unsigned k, size_t usable, const uint8_t delta[32],
                             uint8_t* sigma_lagrange, uint8_t* sigma_coeff);
int h2agg_commit_columns(h2agg_ctx* ctx, uint64_t bases_handle, const uint8_t* columns, size_t m, unsigned k, uint8_t* out_aff);

/* ---- Witness check: which gate, lookup or copy constraint a witness fails, and on which rows ------------------------------
 * Stand for: the gate, lookup and permutation checks of dev::MockProver::verify of halo2_proofs — recalled from upstream, not
 * pinned, like the blocks above; what the entry points compute is this definition.  The order of the constraints IS pinned:
 * halo2-snark-aggregator-api/src/systems/halo2/params.rs:74-224 (gates, then the permutation, then every lookup).
 *
 * Slabs (advice, fixed, instance: Lagrange values, [columns][n]) and challenges are those of h2agg_vk_expressions_eval; n = 2^k
 * and u = n - blinding_factors - 1 are the key's.  Host buffers, synchronous.
 *
 * Constraints are numbered 0 .. C-1, C = G + P + L (h2agg_witness_check_layout gives the three): first the G gate polynomials
 * in key order, gate by gate and poly by poly (the list of which = 0), then the P permutation columns g = 0 .. P-1, then the
 * L lookups.  `what` is a set of H2AGG_WC_* bits: the kinds to check.
 *   counts[C]           the number of failing rows of each constraint
 *   first_rows[C]       its lowest failing row, or 0xFFFFFFFF if there is none
 *   rows[C][max_rows]   the lowest min(count, max_rows) failing rows of each constraint in ascending order, the rest of the
 *                       line 0xFFFFFFFF; rows may be NULL and max_rows may be 0: no rows are reported
 *   total               the sum of the counts
 * A constraint whose kind is not in `what` reports 0 / 0xFFFFFFFF / an empty line.  The call returns H2AGG_OK whether or
 * not anything fails: the report is the result.
 * What "fails" means:
 *   gate polynomial E, row i < u:  E(row i) != 0 in Fr.  Leaves and rotations are exactly those of h2agg_vk_expressions_eval:
 *     rows wrap mod n, so a rotation may read a blinding row.  Rows from u up are never reported.
 *   permutation column g, row i < n:  with v(c, r) the value of the key's permutation column c at row r (taken from the
 *     advice / fixed / instance slab the key names for it) and {c', r'} = mapping[g][i] (the mapping of
 *     h2agg_permutation_assembly / h2agg_permutation_sigmas over the key's P columns): v(g, i) != v(c', r').  In a cycle
 *     a -> b -> c -> a with b's value changed, cells a and b fail and c does not.
 *   lookup j, row i < u:  with A and S the theta-folds of its input and table expressions (h2agg_vk_expressions_eval with
 *     fold = theta, which = 1 / 2): A[i] does not occur among S[0..u) — the predicate h2agg_lookup_permute refuses on, per
 *     row.  For a one-expression lookup this is MockProver's tuple test exactly; for a longer tuple it is the test on the
 *     folds: a row whose tuple is absent passes only if its fold collides with a table row's, which for a theta drawn
 *     after the witness happens with probability at most (tuple length - 1) u / r per row.
 * mapping is read iff H2AGG_WC_PERMUTATION is set and P > 0, theta iff H2AGG_WC_LOOKUPS is set and L > 0 (they may be NULL
 * otherwise).  Every column element a requested check reads is checked for < r.
 *
 * Work memory, kept in the context: one BIT per (constraint, row) — never a value per (constraint, row) —
 * for at most 2^24 flag words (64 MiB) at a time: a key with more than 2^29 / n gate polynomials or permutation columns (32
 * at k = 24) is run in chunks of that many; the 32-bit sums and minima of 2048-row tiles; two columns per lookup call; the
 * sort's work memory of h2agg_lookup_permute; the staged slabs and mapping.  Only the report crosses back to the host:
 * (2 + max_rows) C words and the total.  With the debug key "phases" h2agg_last_phases gives " gates=ms permutation=ms
 * lookups=ms report=ms".
 * Refusals, the context stays usable after each: a null vk, context or required buffer (counts, first_rows and total are
 *   required), what == 0 or an unknown bit in it, a mapping entry with c' >= P or r' >= n (scanned on the host), an expression
 *   of a requested kind deeper than H2AGG_EXPR_MAX_DEPTH: H2AGG_ERR_INVALID.  A scalar (challenge, theta, a CONST of the key)
 *   >= r: H2AGG_ERR_NONCANONICAL from the call.  A column element >= r: H2AGG_ERR_NONCANONICAL through the context's device
 *   status, from the call; the outputs are then unspecified.  Out of memory: H2AGG_ERR_NOMEM.
 *
 * The resident form is h2agg_columns_witness_check, over column stores. */
#define H2AGG_WC_GATES 1
#define H2AGG_WC_PERMUTATION 2
#define H2AGG_WC_LOOKUPS 4
int h2agg_witness_check_layout(const h2agg_vk* vk, size_t* n_gate_polys, size_t* n_perm_columns, size_t* n_lookups);
int h2agg_witness_check(h2agg_ctx* ctx, const h2agg_vk* vk, unsigned what, const uint8_t* advice, const uint8_t* fixed,
                        const uint8_t* instance, const uint8_t* challenges, const uint8_t theta[32], const uint32_t* mapping,
                        size_t max_rows, uint32_t* counts, uint32_t* first_rows, uint32_t* rows, uint64_t* total);

/* ---- Fr column stores: prover columns that stay on the device between stages -------------------------------------------------
 * What h2agg_bases_upload / h2agg_g1_msm_preloaded are to G1 bases, for scalars: a store is a slab [m][n] of canonical 32-byte
 * little-endian Fr elements, n = 2^k, column j at byte 32 * n * j, in DEVICE memory that the context owns behind a handle
 * (handles are never 0 and never reused; a store's handle is no base table's).  A caller without HIP of its own writes its
 * witness once, runs the stages over stores and reads back only commitments, evaluations and reports.  The families that take
 * whole slabs have resident forms below; every other family runs over a store through its _device entry point and
 * h2agg_columns_ptr.  Each resident form answers byte for byte what its host-buffer family answers, keeps that family's
 * definitions and refusals, and changes only where the columns live.
 *
 * Buffer rules.  A store's memory is the library's, ordered on the context's stream: everything below is queued there, and a
 * call synchronises only where results go to host memory (said per call).  h2agg_set_stream: the stores follow the rule the
 * base tables and the context's work memory follow — the switch joins and waits for everything queued on the old stream, so a
 * store is complete when h2agg_set_stream returns and is ordered on the new stream from then on; nothing is copied or moved.
 *
 * h2agg_columns_create   allocates exactly 32 * m * n bytes, zero-filled; *handle_out names the store.
 * h2agg_columns_destroy  waits for the work queued on the context and frees the slab.  h2agg_destroy frees every store that
 *   is left, as it frees the base tables.
 * h2agg_columns_info     m and k of a store (either output may be NULL).
 * h2agg_columns_write    columns first .. first + count - 1 from host memory (pageable or from h2agg_host_alloc; count * n
 *   elements); synchronous.  Every element written is checked: one >= r gives H2AGG_ERR_NONCANONICAL from the call, the written
 *   columns are then unspecified (write them again), the other columns and the context are as before.  With the debug key
 *   "phases" h2agg_last_phases gives " stage=ms check=ms": the copy and the check of the elements.
 * h2agg_columns_read     the same range back to host memory; synchronous.
 * h2agg_columns_ptr      the device address of column `first`, valid until the store is destroyed: what the _device entry
 *   points take (columns first, first + 1, ... follow at 32 * n bytes each).  The memory is ordered on the context's stream,
 *   which is exactly what the buffer rules of the _device entry points ask of a caller's buffers: handing the pointer to
 *   them needs no synchronisation.  A caller that touches the memory with HIP of its own orders that work against the
 *   context's stream itself.
 * h2agg_columns_move     dst[dfirst + j][i] = src[sfirst + j][(i + rotation) mod n] for j < count, with the mathematical
 *   modulus: any int32 rotation is legal, -1 reads the row before.  Queued.  The two stores must have one k.  One store on both
 *   sides is allowed when the two column ranges are disjoint, or when they are the same range and rotation mod n == 0 (nothing
 *   is done); any other overlap: H2AGG_ERR_INVALID.
 *
 * Resident forms.
 * h2agg_columns_fft      h2agg_fr_fft_batch over `count` columns, k the stores'; queued, no synchronisation (a workspace that
 *   has to grow drains the device first, as for h2agg_fr_fft_device).  In place is allowed: dst == src with dfirst == sfirst.
 *   Any other overlap of the two ranges and stores of different k: H2AGG_ERR_INVALID.  An element >= r raises the context's
 *   device status, as for h2agg_fr_fft_device.
 * h2agg_columns_commit   h2agg_commit_columns over `count` columns with no staging; synchronous (the points go to the host).
 * h2agg_columns_sigmas   h2agg_permutation_sigmas with the two outputs in stores: the Lagrange columns to columns lfirst ..
 *   lfirst + m - 1 of dst_lagrange, the coefficient columns to cfirst .. of dst_coeff.  Either handle may be 0 (that output
 *   is not wanted), not both; the two ranges must not overlap.  The mapping comes from host memory.  Synchronous up to the
 *   device's verdict on the mapping: an invalid mapping is H2AGG_ERR_INVALID from the call and leaves both stores unchanged
 *   (the columns are made in work memory and reach the stores by a device copy queued behind the verdict).
 * h2agg_columns_witness_check  h2agg_witness_check with the three slabs in stores: the key's num_advice columns from afirst
 *   of `advice`, its fixed columns from ffirst of `fixed`, its instance columns from ifirst of `instance`; a handle is not
 *   looked at where the key has no column of the kind.  mapping, challenges, theta and the report are host memory, as there;
 *   the report's layout is unchanged.  Synchronous.
 * h2agg_columns_shplonk_begin  h2agg_kzg_shplonk_begin over columns first .. first + npoly - 1 of a store, k the store's.
 *   Returns the same object: h2agg_kzg_shplonk_finish and _destroy are the existing ones.  The object's own slab is filled by
 *   a device copy of the store's columns inside the call, so the store may be overwritten or destroyed before _finish.
 *
 * Refusals common to all, H2AGG_ERR_INVALID with the context usable and no output written: an unknown or destroyed handle;
 * first + count (npoly, m, the key's column count) beyond the store's m, or count == 0; a store whose k is not the call's, the
 * other store's or the key's; m == 0 or k > 24 at create; a null host buffer.  A slab whose byte size does not fit size_t:
 * H2AGG_ERR_NOMEM without an allocation; a failed allocation: H2AGG_ERR_NOMEM.  The context stays usable after each. */
int h2agg_columns_create(h2agg_ctx* ctx, size_t m, unsigned k, uint64_t* handle_out);
int h2agg_columns_destroy(h2agg_ctx* ctx, uint64_t handle);
int h2agg_columns_info(h2agg_ctx* ctx, uint64_t handle, size_t* m_out, unsigned* k_out);
int h2agg_columns_write(h2agg_ctx* ctx, uint64_t handle, size_t first, size_t count, const uint8_t* host);
int h2agg_columns_read(h2agg_ctx* ctx, uint64_t handle, size_t first, size_t count, uint8_t* host);
int h2agg_columns_ptr(h2agg_ctx* ctx, uint64_t handle, size_t first, void** d_ptr_out);
int h2agg_columns_move(h2agg_ctx* ctx, uint64_t src, size_t sfirst, uint64_t dst, size_t dfirst, size_t count, int32_t rotation);
int h2agg_columns_fft(h2agg_ctx* ctx, uint64_t src, size_t sfirst, uint64_t dst, size_t dfirst, size_t count, int inverse,
                      const uint8_t shift[32]);
int h2agg_columns_commit(h2agg_ctx* ctx, uint64_t bases_handle, uint64_t src, size_t first, size_t count, uint8_t* out_aff);
int h2agg_columns_sigmas(h2agg_ctx* ctx, const uint32_t* mapping, size_t m, unsigned k, size_t usable, const uint8_t delta[32],
                         uint64_t dst_lagrange, size_t lfirst, uint64_t dst_coeff, size_t cfirst);
int h2agg_columns_witness_check(h2agg_ctx* ctx, const h2agg_vk* vk, unsigned what, uint64_t advice, size_t afirst, uint64_t fixed,
                                size_t ffirst, uint64_t instance, size_t ifirst, const uint8_t* challenges, const uint8_t theta[32],
                                const uint32_t* mapping, size_t max_rows, uint32_t* counts, uint32_t* first_rows, uint32_t* rows,
                                uint64_t* total);
int h2agg_columns_shplonk_begin(h2agg_ctx* ctx, uint64_t g_handle, uint64_t src, size_t first, size_t npoly, const uint32_t* queries,
                                size_t nq, const uint8_t* points, size_t npoints, const uint8_t* evals, const uint8_t y[32],
                                const uint8_t v[32], uint8_t h1_aff[64], h2agg_shplonk** out);

/* ---- Proving key on the device: the forms a prover of one circuit keeps between proofs ---------------------------------------
 * Stands for: what halo2_proofs' ProvingKey caches — fixed_values / fixed_polys / fixed_cosets, the permutation's permutations /
 * polys / cosets, and l0, l_last, l_active_row — recalled from upstream, not pinned, like the blocks above; what the entry
 * points compute is this definition.  None of it depends on a witness or a challenge, and h2agg_quotient* recomputes all of
 * it in every call: the three Lagrange columns once, the transforms of the key's columns on every coset.  A prover that proves
 * one circuit many times (the aggregator's own case) builds the object once and calls h2agg_pk_quotient.
 *
 * Elements are canonical 32-byte little-endian Fr.  n = 2^k is the key's, F = its fixed commitments, P = its permutation
 * columns; e, w_ext, zeta, u, l_0, l_last, l_blind are those of h2agg_quotient; coset c' < 2^e is the shift s = zeta w_ext^c'.
 *
 * h2agg_pk_create — fixed[F][n] and sigma[P][n] are host slabs in LAGRANGE form (a slab whose count is zero may be NULL); sigma
 *   is what h2agg_permutation_sigmas writes to sigma_lagrange.  Synchronous: when it returns every form is complete in device
 *   memory that the object owns.  The object refers to ctx and vk, which must outlive it.  forms: 0 or H2AGG_PK_COSETS.
 * h2agg_pk_create_resident — the same with the two slabs in DEVICE memory (for example h2agg_columns_ptr of a store); the
 *   buffer rules of h2agg_fr_fft_device apply, the inputs are not written, and it still returns only when the forms are complete.
 * The forms:
 *   always  the Lagrange form as given;
 *   always  the coefficient form: one batched inverse transform, byte for byte what h2agg_fr_fft_batch (inverse, no shift)
 *           gives — for sigma what h2agg_permutation_sigmas writes to sigma_coeff;
 *   always  l_0, l_last, l_blind in coefficient form: the inverse transforms of the rows (i == 0), (i == u), (i > u);
 *   with H2AGG_PK_COSETS, for every coset c' one slab [F + P + 3][n]: the values on {s w^i} of the fixed polynomials, then the
 *           sigma polynomials, then l_0, l_last, l_blind — one batched forward transform at shift s, every column byte for
 *           byte what h2agg_fr_fft_device gives for it.
 *   Without that bit the object is the low-memory key: h2agg_pk_quotient transforms the key's columns per coset from the
 *   coefficient forms, as h2agg_quotient_device does, and saves only the per-call construction of the three columns.
 * h2agg_pk_bytes — the device memory the object will hold:
 *       32 x (2 (F + P) n + 3 n + [H2AGG_PK_COSETS] (F + P + 3) n 2^e)  bytes
 *   (k = 24, F + P = 12, e = 2: 12 + 1.5 + 30 GiB).  Needs no context and no device, like h2agg_quotient_work_bytes, and
 *   refuses the same shapes.
 * h2agg_pk_info — k, e, F, P, forms and the bytes held; every output may be NULL.
 * h2agg_pk_ptr — a read-only device pointer to one form and its number of columns, for the _device entry points:
 *   H2AGG_PK_FIXED_LAGRANGE [F][n] (h2agg_vk_expressions_eval_device, the witness check), H2AGG_PK_SIGMA_LAGRANGE [P][n]
 *   (h2agg_permutation_product_device), H2AGG_PK_FIXED_COEFF / H2AGG_PK_SIGMA_COEFF (h2agg_fr_poly_eval_device, the multiopen
 *   slabs, h2agg_quotient_device), H2AGG_PK_LAGRANGE_COEFF [3][n]: l_0, l_last, l_blind, and H2AGG_PK_COSET: the slab
 *   [F + P + 3][n] of coset `coset` (ignored for the other forms).  A form without columns answers NULL and 0 columns.
 * h2agg_pk_quotient — h2agg_quotient_device with the key's polynomials taken from the object: device memory in and out, queued
 *   on the context's stream, no synchronisation and no read-back (a workspace that has to grow drains the device first).
 *   d_h is byte for byte what h2agg_quotient_device writes for the same witness polynomials and the object's FIXED_COEFF and
 *   SIGMA_COEFF slabs, on both endings (k + e <= 24; the coset-split ending above that and under h2agg_quotient_configure).
 *   With H2AGG_PK_COSETS nothing moves a key column, per coset or per call: the kernels read the object's coset slabs in
 *   place, and the one batched transform per coset takes the witness alone.
 *   Work memory, kept in the context, with H2AGG_PK_COSETS: (A + I + sets + 3 L + 3) n + 2^(k+e) elements (the witness slab of
 *   a coset, the fold column, a lookup's two theta-folds, the extended evaluations or the cosets' inverse transforms) and the
 *   transforms' work array by h2agg_fr_fft_batch's rule for A + I + sets + 3 L columns of n, raised to 2^(k+e) elements on the
 *   default ending.  Without the bit: h2agg_quotient's two sums less the three coefficient columns.  A key with no witness
 *   column at all is legal and transforms nothing per coset.
 *   h2agg_last_phases (debug key "phases") gives the five names of h2agg_quotient_device; forward is the witness transforms.
 * h2agg_pk_quotient_work_bytes — that work memory in bytes, on the route the key takes by its size (as
 *   h2agg_quotient_work_bytes).
 * h2agg_pk_destroy — waits for the context's stream, then frees.  NULL does nothing.
 * Refusals, the context stays usable after each and create leaves *out = NULL: a shape h2agg_quotient_device refuses (k > 24,
 *   k + e > 28, degree < 3 with permutation columns), a null required buffer, unknown bits in forms, a key used with another
 *   context, an unknown `which`, coset >= 2^e or H2AGG_PK_COSET asked of a key built without the bit: H2AGG_ERR_INVALID.  An
 *   element >= r in fixed or sigma: H2AGG_ERR_NONCANONICAL from create.  A scalar >= r: H2AGG_ERR_NONCANONICAL from the call.  A
 *   witness element >= r: H2AGG_ERR_NONCANONICAL through the context's device status, as for h2agg_quotient_device.  Out of
 *   memory: H2AGG_ERR_NOMEM, with nothing left allocated. */
#define H2AGG_PK_COSETS 1u
#define H2AGG_PK_FIXED_LAGRANGE 0
#define H2AGG_PK_SIGMA_LAGRANGE 1
#define H2AGG_PK_FIXED_COEFF 2
#define H2AGG_PK_SIGMA_COEFF 3
#define H2AGG_PK_LAGRANGE_COEFF 4
#define H2AGG_PK_COSET 5
typedef struct h2agg_pk h2agg_pk;
int h2agg_pk_create(h2agg_ctx* ctx, const h2agg_vk* vk, const uint8_t* fixed, const uint8_t* sigma, unsigned forms, h2agg_pk** out);
int h2agg_pk_create_resident(h2agg_ctx* ctx, const h2agg_vk* vk, const void* d_fixed, const void* d_sigma, unsigned forms,
                             h2agg_pk** out);
int h2agg_pk_bytes(const h2agg_vk* vk, unsigned forms, size_t* bytes_out);
int h2agg_pk_info(const h2agg_pk* pk, unsigned* k_out, unsigned* e_out, size_t* fixed_out, size_t* sigma_out, unsigned* forms_out,
                  size_t* bytes_out);
int h2agg_pk_ptr(const h2agg_pk* pk, int which, size_t coset, const void** d_ptr_out, size_t* columns_out);
int h2agg_pk_quotient(h2agg_ctx* ctx, const h2agg_pk* pk, const void* d_advice, const void* d_instance, const void* d_perm_z,
                      const void* d_lookup_z, const void* d_lookup_ap, const void* d_lookup_sp, const uint8_t* challenges,
                      const uint8_t theta[32], const uint8_t beta[32], const uint8_t gamma[32], const uint8_t y[32],
                      const uint8_t delta[32], void* d_h);
int h2agg_pk_quotient_work_bytes(const h2agg_pk* pk, size_t* bytes_out);
void h2agg_pk_destroy(h2agg_pk* pk);

/* ---- Fr expression tape ------------------------------------------------------
 * A straight-line program over Fr, run on the device by the interpreter EvaluationQuerySchema::eval records into:
 * registers 0 .. nconst-1 are the inputs (canonical, 32 B each), register nconst + k is the result of op k;
 * ops3 = nops x {opcode, a, b} (u32 each; opcode 0 = mul, 1 = add, 2 = sub, 3 = inverse of a (b ignored; 1/0 -> H2AGG_ERR_DIV_ZERO, the `invert().unwrap()` of MockFieldChip::div); a, b < nconst + k).  Independent ops run in
 * parallel, a chain costs one multiplication latency per link.  out_regs selects the nout registers returned in `out`
 * (canonical).  This is the shape of the verifier's scalar-side expressions (halo2-snark-aggregator-api/src/systems/halo2/
 * {params,lookup,permutation,vanish,lagrange,expression}.rs evaluate such programs through ArithFieldChip). */
int h2agg_fr_tape_eval(h2agg_ctx* ctx, const uint8_t* consts, size_t nconst, const uint32_t* ops3, size_t nops,
                       const uint32_t* out_regs, size_t nout, uint8_t* out);

/* ---- tuning / measurement -------------------------------------------------------------------------
 * window_bits: Pippenger window c in [2, 20]; 0 = the measured table (GLV: 8 / 13 / 16 for n <= 2^10 / <= 2^14 / larger;
 * plain: 8 / 15 / 16 for n <= 2^12 / < 2^19 / larger — wide windows with a uniform top window).
 * reduce_segment: buckets per running-sum segment of the bucket reduction (power of two; 0 = 2 / 4 / 8 by bucket count,
 * 32 for n >= 2^20 in overlap mode).  big_bucket_threshold: run length above which a bucket is cut into
 * workgroup-sized chunks (0 = max(256, 8 x mean)). */
int h2agg_msm_configure(h2agg_ctx* ctx, int window_bits, int reduce_segment, int big_bucket_threshold);
/* (16-bit windows reduce their buckets as 256 rows x 128 columns — plain sums, then two weighted sums per window — unless
 * reduce_segment is given, which selects the running-sum segment kernels; a -DH2AGG_MEASURE_KNOBS build also reads H2AGG_REDUCE=segments.) */
/* GLV / endomorphism split of the scalars (k = k1 + lambda*k2, |k_i| < 2^127; phi(P) = (beta*x, y)): halves the
 * number of windows — same bucket additions, half the bucket reduction and half the serial doubling chain.
 * beta*x is computed once per base (a 32 B/point column beside the table), so the price is the decomposition pass and
 * the slice-combine pass of the half-as-many buckets: mode 0 = auto turns it on unless the tail is hidden anyway
 * (overlap mode and n >= 2^20) or is a small share of the work (n >= 2^22); 1 = on, -1 = off (254-bit windows). */
int h2agg_msm_configure_glv(h2agg_ctx* ctx, int mode);
/* Lanes per bucket in the accumulation kernel (1, 2, 4, 8, 16; 0 = chosen so that ~8192 waves are launched, at most 8
 * and at most the mean bucket occupancy). */
int h2agg_msm_configure_lanes_per_bucket(h2agg_ctx* ctx, int lanes);
/* Bucket-sort knobs: low bucket bits resolved per partition in LDS (4..12) and scalars per level-1
 * workgroup; 0 = default.  tile = -1 forces the two-array direct sort kernels (otherwise used only when
 * n does not fit the packed item's index field, n > 2^(31 - sub_bits)); tile = -2 additionally stages level 1
 * through LDS (measured slower; kept as a tested variant); tile = -3 keeps the packed two-level sort where the
 * digit-major sort would apply (plain 16-bit windows over one table, 2^16 .. 2^22 points; any non-default knob
 * here selects the packed kernels as well).  (A -DH2AGG_MEASURE_KNOBS build also reads H2AGG_SORT=packed.) */
int h2agg_msm_configure_sort(h2agg_ctx* ctx, int sub_bits, int tile);
/* Environment.  The library reads these variables and no others (experiment switches exist only in builds with
 * -DH2AGG_MEASURE_KNOBS, which no shipped library is):
 *   H2AGG_HOST_THREADS=n      worker threads of the host sponge pool (default: the usable cores)
 *   H2AGG_TRANSCRIPT=device|host, H2AGG_HOST_SPONGE=ifma|portable   overrides of h2agg_transcript_configure's automatic choice
 *   H2AGG_NO_PLACE            skip the stream-placement probe of h2agg_create / h2agg_set_stream (needed when the caller's
 *                             stream is being graph-captured: the probe launches and synchronises)
 *   H2AGG_TRACE, H2AGG_TRACE_PHASES   diagnostics on stderr (schema evaluation / phases of h2agg_verify_aggregation)
 *   H2AGG_RCCL_LIB=path       the RCCL build to dlopen for the comm entry points instead of the librccl.so.1 already in the
 *                             process / on the loader path (an operator's own build; tests point it at their stand-in)
 *   H2AGG_PAIRING_PORTABLE    (any value) the host pairing in its portable build even on a CPU with BMI2 + ADX (A/B of the two
 *                             instantiations of csrc/pairing.hpp; the pairing entry points take ctx = NULL, so this is not a key)
 * Test hooks, per context and per call (tests/ exercise code paths a production call reaches only by size):
 *   key "pcie_slices" n   cut h2agg_g1_msm's host buffers into n slices (0 = automatic)
 *       "pcie_glv" -1|0|1 GLV for those slices (0 = automatic)       "pcie_chain" 0|1  slices share one bucket set (default 1)
 *       "comb_msm" 0|1    small MSMs over tables with fixed-base levels take the comb (default 1)
 *       "plan_cache" 0|1  h2agg_verify_aggregation keeps the recording of a call shape (default 1)
 *       "small_sort" 0|1  MSMs of <= 16384 scalars sort in one launch (default 1; 0 = the packed two-level sort)
 *       "eval_split" 0|1  the two multi_exps of an evaluation run as one set of launches (default 1)
 *       "lean_acc" 0|1    bucket accumulation through k_msm_accumulate_lean (default 1; 0 = the generic kernel, which only the
 *                         measure build carries: the shipped library answers H2AGG_ERR_INVALID)
 *       "tape_lds" 0|1    Fr tapes whose live values fit run with the register file in LDS (default 1; 0 = through L2)
 *       "prewake" 0|1     a from-bytes call wakes its sponge workers at entry (they spin until the chains are posted), one more
 *                         for the pairing's second Miller loop, and waits only for the element streams in front of the sponges
 *                         (default 1; 0: the three latency measures of round 6 off, for an A/B)
 *       "phases" 0|1      keep every aggregation call's wall-clock split, and every h2agg_kzg_multiopen* call's split by events
 *                         (combine / divide / commit) and every h2agg_quotient* call's (forward / gates / permutation / lookups /
 *                         inverse; the queued form then waits for its own events) and every h2agg_permutation_sigmas call's
 *                         (stage / sigma / inverse / copy) and every h2agg_witness_check call's (gates / permutation / lookups /
 *                         report) and every h2agg_kzg_shplonk_begin / _finish call's (stage / numerators / divide / commit;
 *                         combine / divide / commit), for h2agg_last_phases
 *       "fr_fft_local" L  h2agg_fr_fft / _device fuse L radix-2 stages per pass, 1 .. 11 (0 = the default, 10): inputs of 8 to
 *                         1024 elements then run the multi-pass paths
 *       "fr_fft_batch_chunk" B  a batched transform (h2agg_fr_fft_batch, the transforms inside h2agg_quotient) runs in chunks of
 *                         B columns, every pass of a chunk one launch (0 = the default: as many columns as the work array holds)
 *       "fr_poly_chunk" t the KZG opening kernels cut a polynomial into chunks of 2^t coefficients per workgroup, 3 .. 11 (0 = the
 *                         default, 11): inputs of 64 to 1024 coefficients then run the three- and four-level plans (the
 *                         Shplonk prover's sweeps and set division take the same cut)
 *       "fr_scan_chunk" t the grand-product kernels (batch inversion, running product) cut an array into chunks of 2^t elements
 *                         per workgroup, 3 .. 11 (0 = the default, 11): inputs of 64 to 1024 rows then run the three- and
 *                         four-level plans
 *       "fr_sort_tile" t  h2agg_lookup_permute sorts and ranks in tiles of 2^t keys per workgroup, 4 .. 11 (0 = the default, 11);
 *                         below 11 the step of its row scans, the threads that take keys in its byte histogram (both 2^(t-2))
 *                         and that histogram's grid (2 workgroups) shrink with the tile: at t = 4 inputs of 65 to 1024 rows
 *                         then run every multi-tile path, the step loops of both scans and the histogram's stride loop included
 *       "commit_chunk" B  h2agg_commit_columns hands its columns to the batched MSM B at a time (0 = the default: as many as hold
 *                         2^22 scalars): a slab of a few short columns then crosses the chunk boundary
 *       "launch_cus" u    the grid-stride launches whose workgroup cap goes by the device (u x 8 workgroups of 256 elements for
 *                         the element-wise kernels, u x 16 of 32 points for h2agg_g1_batch_scalar_mul and the comb's table, u x 4,
 *                         u x 12 and u x 8 for the MSM's size order, fix-up and over-long-bucket lists) count u compute units,
 *                         1 .. 1024 (0 = the default: the device's own count).  Sizes grids only: routes, plans, lanes per bucket
 *                         and stream placement keep the real count.  At u = 1 an input of a few thousand elements walks every
 *                         such loop several times
 *       "lean_full" 0|1   the bucket accumulation keeps its per-entry identity test and endomorphism select for every table
 *                         and plan (1: A/B and tests of the instantiation for any table)
 *       "pre_big" 0|1     h2agg_bases_precompute takes any explicit width (1: levels through the two-array sort, A/B only)
 *       "seg_chunk" n     h2agg_g1_msm_segmented / h2agg_verify_proofs: at most n points per set of launches of the segmented
 *                         multi_exp (0 = automatic, 16384); a segment longer than that is an ordinary multi_exp of its own
 *       "seg_c" 4..8      window bits of the segmented multi_exp (0 = the default, 5; measurement only)
 *       "shard_fail" 0..4  this rank of h2agg_verify_aggregation_sharded fails before (1) / between (2) its exchanges, or inside
 *                         exchange 1 (3) / 2 (4) before its all-gather */
int h2agg_debug_configure(h2agg_ctx* ctx, const char* key, int value);
/* The bucket accumulation has one instantiation per (table may hold the identity, plan has endomorphism entries): the two
 * per-entry decisions it then leaves out are properties of the call (csrc/msm_kernels.hpp LEAN_ID = 1, LEAN_ENDO = 2).
 * h2agg_debug_lean_variant: the set a call takes, from what is known of its table and plan; needs no device.
 * h2agg_debug_table_identity: *may_hold_out = 0 when the call that wrote the table (h2agg_bases_upload / _generate / _fft,
 * h2agg_params_setup) stored no identity base, 1 otherwise ("may hold one": also every table that was not written by one of
 * them); *last_variant_out = the set of the context's last bucket accumulation, -1 before the first.  Either pointer may be NULL
 * (handle is only looked up for may_hold_out).  h2agg_debug_configure(ctx, "lean_full", 1) makes every call take the full set. */
int h2agg_debug_lean_variant(int table_no_identity, int plan_glv);
int h2agg_debug_table_identity(h2agg_ctx* ctx, uint64_t handle, int* may_hold_out, int* last_variant_out);
/* Overlap the latency-shaped tail of one MSM (enable = 1: the Horner kernel, one wave; 2: bucket reduction + window
 * sums + Horner; 3: as 2, and the bucket accumulation itself leaves the context's stream, so that the NEXT MSM's sort runs
 * under it — measured: a loss at 2^20 points (1.39 -> 1.55 ms per MSM: both kernels slow each other down), +3 % at 2^22) with the bulk kernels of the next ones: the tail runs on one of three tail streams of the context.  With overlap on, a result written by
 * h2agg_g1_msm_device_async is complete after h2agg_synchronize() (or after the next synchronous call on
 * the context), not merely after the caller's stream has drained: from 2^20 points on, the tail of the LAST MSM queued is only launched by
 * the next call on the context (behind that MSM's sort, where it costs least) or by h2agg_synchronize(); smaller MSMs launch
 * theirs at once (there the tail is a large share of the MSM: waiting costs more than the next sort gains).  Default: off. */
int h2agg_msm_set_tail_overlap(h2agg_ctx* ctx, int enable);
/* When enabled, every MSM stage is bracketed by HIP events on the context's stream and per-stage times
 * are accumulated.  enable: 0 = off, 1 = every stage, 2 + s = only stage s (one event pair per MSM: the event
 * packets between kernels cost ~5 us each, which is 5-8 % of a 2^20 MSM when all nine stages are bracketed). */
int h2agg_profile_enable(h2agg_ctx* ctx, int enable);
int h2agg_profile_reset(h2agg_ctx* ctx);
/* Number of stages; name of stage i; accumulated milliseconds and launch count of stage i. */
int h2agg_profile_stage_count(h2agg_ctx* ctx);
const char* h2agg_profile_stage_name(h2agg_ctx* ctx, int i);
int h2agg_profile_stage_get(h2agg_ctx* ctx, int i, double* total_ms, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* H2AGG_H */
