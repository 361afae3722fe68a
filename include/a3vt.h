/* a3vt.h — C ABI of the MI355X (gfx950) mesh-reconstruction hot path.
 *
 * Drop-in boundary for the reconstruction path of facebookresearch/Active-3D-Vision-and-Touch
 * (`pterotactyl`).  The reference has no native/FFI layer: its boundary is the
 * Python module API of pterotactyl.reconstruction.vision.{model,train} and pterotactyl.utility.utils,
 * which reach third-party kernels through torch / PyTorch3D.  Every entry point below names the
 * reference call site (file:line under /root/reference) whose arithmetic it replaces; the Python
 * façade in active-3d-vision-and-touch_amd/pterotactyl/ binds them with ctypes.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch types.  Return 0 = OK, <0 = error
 *    (a3vt_last_error() gives a thread-local message).
 *  - All data pointers are caller-owned DEVICE pointers unless a parameter says "host".
 *    The library never allocates or frees user tensors and never synchronises the host;
 *    scratch memory comes from the caller (query with the *_bytes functions).
 *  - `stream` is a hipStream_t (NULL = default stream).  Everything is fp32; indices are int32.
 *  - Dense row-major layouts.  M = batch * n_vert rows of per-vertex data, sample-major.
 */
#ifndef A3VT_H
#define A3VT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A3VT_VERSION 163 /* 163: a3vt_adam_step (the trainer's Adam step over all parameter tensors in one launch); 162: a3vt_conv5_weight_grad (the weight gradients of the image pyramid's 5 x 5 layers: fixed-order sums, no fill / cast launches); 161: a3vt_bnrelu_fwd / _bwd (training BatchNorm2d + ReLU of the image pyramid on channels-last bf16 maps), a3vt_cast_weights_bf16, a3vt_image_pool_fwd_add, a3vt_conv5_nhwc; 160: a3vt_adj_split, a3vt_adj_split_validate, a3vt_gcn_stack_fwd_adj / _bwd_adj (the fused vision + touch adjacency as P + a complete bipartite block); 150: a3vt_dbg_path_counts, larger a3vt_chamfer_workspace_bytes (oriented boxes of the pruned search), a3vt_gcn_stack_scratch_bytes covers every gemm mode, gemm_bf16 outside 0..3 refused; 140: gemm_bf16 = 3 ("fp32x3": fp32 products as six bf16 MFMA passes on exactly split operands), a3vt_split3_bf16; 0.2.x: bf16 storage mode (gemm_bf16 = 2), a3vt_gcn_stack_stash_bytes / _scratch_bytes_mode, deterministic backward scatters; 120: a3vt_chamfer_fwd_ws (pruned exact search); 130: a3vt_posenc_wide_* (448-wide vertex-feature encoder), larger a3vt_gcn_stack_mask_bytes / _scratch_bytes (channel-sliced aggregation) */

int a3vt_version(void);
const char *a3vt_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Adjacency.  Replaces the dense (N,N) float adjacency of utility/utils.py:47-52,134-148 with CSR
 * (row-normalised, self loops included).  Host-side structural check: monotone rowptr, columns in
 * range.  Pointers are HOST pointers.  */
int a3vt_csr_validate(const int32_t *rowptr_host, const int32_t *col_host, int n_vert, int nnz);

/* ---------------------------------------------------------------------------------------------
 * GCN.  Replaces GCN_layer.forward, reconstruction/vision/model.py:351-363
 *   Z = X W ;  Y[:, :c] = A Z[:, :c] + b[:c] ;  Y[:, c:] = Z[:, c:] ;  ReLU     (hidden layers, do_cut)
 *   Y = A (X W) + b                                                              (last layer, 3 channels)
 * and GCN.forward, model.py:316-331 (the layer loop; the NaN trap at :326 becomes a3vt_check_finite).
 *
 * Layer dims follow model.py:297-301: [in_features, hidden x (L-1), 3].  `weights[i]` is the
 * reference parameter layout (1, in_i, out_i) = row-major [in_i][out_i]; `biases[i]` is [out_i].
 * `weights`, `biases`, `grad_weights`, `grad_biases` are HOST arrays of L DEVICE pointers.
 * `cut_len` = round(hidden * cut) (model.py:355; 99 for 300 * 0.33).
 * csr_* is A (row-normalised), csrT_* is its transpose (A is not symmetric after normalisation).
 * gemm_bf16 (every GCN entry point and a3vt_rowgemm; 2 = bf16 storage, stack entry points only, see below): 0 = the
 * per-vertex products run as exact fp32 MFMA (the parity
 * mode, BASELINE configs[1]/[2]); 1 = "bf16 + MFMA feature MLP" (configs[3]/[4]): the operands of X W, dZ W^T and
 * X^T dZ are rounded to bf16 on their way into the matrix pipe (v_mfma_f32_16x16x16_bf16, fp32 accumulation); every
 * stored tensor stays fp32.  Vertex positions then agree with the fp32 reference to ~2e-3 relative instead of 3e-7.
 * 3 = "fp32x3" (stack entry points only; csrc/gcn_gemm3.hip): every stored tensor stays fp32 exactly as in mode 0, and
 * the three products of the hidden layers (K, n in (288, 304], >= 12 288 rows) are formed on the bf16 matrix pipe from
 * operands split EXACTLY into three bf16 pieces (x == hi + mid + lo, a3vt_split3_bf16), the six partial products down
 * to 2^-16 of the largest kept, fp32 accumulation: fp32-level error (measured against the fp64 oracle: DESIGN.md), not
 * bit-identical to mode 0; all other shapes of such a call run the mode-0 kernels — and so does the WHOLE stack when its
 * ReLU-sign rows are longer than 128 bytes (pad4(cut_len)/4 + ceil(hidden/4) > 128, i.e. cut_len > 212 at hidden 300): a
 * shape that works in mode 0 works in mode 3.  Mode 3 keeps three bf16 weight images per hidden layer in `scratch`, a
 * larger slot than mode 0's: size the scratch with a3vt_gcn_stack_scratch_bytes (enough for every mode) or with
 * a3vt_gcn_stack_scratch_bytes_mode(..., 3).  Values outside 0..3 are refused (A3VT error).  Mode 0 stays the default.
 * csr_max_degree / csrT_max_degree: the largest number of entries in a row of that matrix, or 0 if unknown.  The
 * fused vision + touch graphs have hub rows (chart centres linked to every seam vertex, ~1150 entries,
 * utility/utils.py:119-128); rows above 64 entries are aggregated by a whole workgroup in a second launch, which a
 * known small maximum lets the library skip.  Results do not depend on the value.  With every row <= 8 entries (the vision
 * templates), fp32 storage, hidden 273-304, <= 3072 vertices per mesh and >= 12 288 rows the forward uses the channel-sliced
 * aggregation (csrc/gcn_csrq.hip) and leaves hybrid rows in the stash; the library remembers which layout it wrote into a
 * stash (keyed by the `masks` pointer) and the backward call that receives that stash follows it, whatever its own hint.
 *
 * feats  : [M][ld_feats] with ld_feats == in_features rounded up to a multiple of 4; pad columns must be zero.
 * acts   : saved inputs of layers 1..L-1, (L-1) * M * hidden floats (needed by the backward pass).  OPAQUE to the caller:
 *          row-major [L-1][M][hidden] on the half-wave aggregation path, "hybrid" rows on the channel-sliced one (per layer
 *          columns [0,160) quad-major [batch][40][n_vert] float4, then columns [160,hidden) row-major) — same size either way
 * masks  : ReLU sign bytes of those activations (1 byte per 4 channels), a3vt_gcn_stack_mask_bytes() bytes (opaque);
 *          the backward pass reads these 16 MB per layer instead of re-reading the 197 MB activation
 * update : [M][3]
 * Forward-only callers (policy scoring, environment.py:221-257) may pass acts = masks = NULL: the
 * layer outputs then ping-pong inside `scratch`.
 * a3vt_gcn_stack_scratch_bytes: enough for ANY gemm_bf16 (the maximum over the modes); a3vt_gcn_stack_scratch_bytes_mode
 * (below) is the exact figure of one mode.  The stack entry points take no scratch size: an undersized scratch is
 * undefined behaviour, so size it with one of the two. */
size_t a3vt_gcn_stack_scratch_bytes(int batch, int n_vert, int in_features, int hidden, int num_layers,
                                    int cut_len, int need_backward);
size_t a3vt_gcn_stack_mask_bytes(int batch, int n_vert, int hidden, int num_layers, int cut_len);
/* gemm_bf16 == 2, "bf16 storage" (BASELINE configs[3]/[4]): activations, their gradients and the weight images are kept
 * as bf16 in HBM (fp32 accumulation; fp32 weights, gradients of the weights, features and update at this boundary).
 * `acts` then holds bf16 rows of pad8(hidden) elements — and, behind them, the stack's input rows in bf16, which the backward
 * reads instead of converting `feats` again — and the sign bytes use another row length: query both sizes
 * with a3vt_gcn_stack_stash_bytes, and the scratch size with a3vt_gcn_stack_scratch_bytes_mode (or the all-modes
 * maximum a3vt_gcn_stack_scratch_bytes).  Needs >= 2 layers. */
size_t a3vt_gcn_stack_scratch_bytes_mode(int batch, int n_vert, int in_features, int hidden, int num_layers,
                                         int cut_len, int need_backward, int gemm_bf16);
int a3vt_gcn_stack_stash_bytes(int batch, int n_vert, int hidden, int num_layers, int cut_len, int gemm_bf16,
                               size_t *acts_bytes, size_t *mask_bytes);

int a3vt_gcn_stack_fwd(const float *feats, int ld_feats, int in_features,
                       const float *const *weights, const float *const *biases,
                       int num_layers, int hidden, int cut_len,
                       const int32_t *csr_rowptr, const int32_t *csr_col, const float *csr_val, int csr_max_degree,
                       int n_vert, int batch, int gemm_bf16,
                       void *acts, uint8_t *masks, float *scratch, float *update, void *stream);

/* Backward of the stack.  grad_update [M][3] -> grad_feats [M][ld_feats] (pad columns written as 0),
 * grad_weights[i] [in_i][out_i], grad_biases[i] [out_i] (overwritten; channels >= cut_len of hidden
 * biases get exact zeros: they are dead parameters in the reference, model.py:358). */
int a3vt_gcn_stack_bwd(const float *feats, int ld_feats, int in_features,
                       const float *const *weights, const float *const *biases,
                       int num_layers, int hidden, int cut_len,
                       const int32_t *csr_rowptr, const int32_t *csr_col, const float *csr_val,
                       const int32_t *csrT_rowptr, const int32_t *csrT_col, const float *csrT_val, int csrT_max_degree,
                       int n_vert, int batch, int gemm_bf16,
                       const void *acts, const uint8_t *masks, const float *grad_update,
                       float *const *grad_weights, float *const *grad_biases, float *grad_feats,
                       float *scratch, void *stream);

/* The same with `accumulate` != 0: the weight and bias gradients are ADDED to what grad_weights[i] / grad_biases[i] hold
 * (each sum is formed first, in the usual fixed order, then added once) — for trainers that let the library write every
 * gradient where it lives (a flat all-reduce bucket) and whose stages share weights (mesh_deform_2, model.py:268,281:
 * the first backward call of a step overwrites, the second accumulates).  grad_feats is always overwritten. */
int a3vt_gcn_stack_bwd_acc(const float *feats, int ld_feats, int in_features,
                           const float *const *weights, const float *const *biases,
                           int num_layers, int hidden, int cut_len,
                           const int32_t *csr_rowptr, const int32_t *csr_col, const float *csr_val,
                           const int32_t *csrT_rowptr, const int32_t *csrT_col, const float *csrT_val, int csrT_max_degree,
                           int n_vert, int batch, int gemm_bf16,
                           const void *acts, const uint8_t *masks, const float *grad_update,
                           float *const *grad_weights, float *const *grad_biases, float *grad_feats,
                           float *scratch, int accumulate, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Structured adjacency (round 6).  The fused vision + touch matrix of utility/utils.py:75-130 links EVERY seam vertex of the
 * chart atlas (:80-84,119-123) to EVERY touch-chart centre (:95-98,124-128), so the matrix of model.py:356,360 is
 *     A^ = D^-1 (P + J):  P a sparse symmetric 0/1 pattern (<= 10 entries per row on the reference's graphs),
 *                         J the COMPLETE bipartite block S x C and C x S (S = seam vertices, C = chart centres, disjoint),
 *                         D = the row sums of P + J   (every non-zero of row i of A^ is 1 / d_i).
 * (A^ Z)_i = (sum_{j in P(i)} Z_j + [i in S] sum_{c in C} Z_c + [i in C] sum_{s in S} Z_s) / d_i: two sums per mesh replace
 * the ~1150-entry centre rows and the 26-30-entry seam rows (75 % of the non-zeros of the 20-chart graph).  A caller that
 * knows the decomposition passes it NEXT TO the full CSR (which the output layer and every fallback path keep using):
 * the hidden layers of a3vt_gcn_stack_fwd_adj / _bwd_adj then aggregate with it wherever the shape allows (fp32 storage: the
 * channel-sliced kernels of csrc/gcn_csrqs.hip under the conditions listed above with max_degree <= 12; bf16 storage: the
 * row walk over P plus the two sums).  Same values up to fp32 rounding (another association of the same sums), not bit for
 * bit.  All pointers DEVICE pointers; the struct itself lives on the host.  Vision-only templates are the special case
 * n_seam = n_centre = 0.  A split is passed whole: a non-NULL `split` with any of its four arrays NULL is refused. */
typedef struct a3vt_adj_split {
  const int32_t *rowptr; /* [n_vert + 1]  CSR of P */
  const int32_t *col;    /* [rowptr[n_vert]]  ascending within a row */
  const float *scale;    /* [n_vert]  1 / d_i = the value of every non-zero of row i of the full matrix */
  const uint8_t *cls;    /* [n_vert]  0 = neither, 1 = in S, 2 = in C */
  int32_t max_degree;    /* longest row of P */
  int32_t n_seam, n_centre;
} a3vt_adj_split;

/* Host-side proof that (P, S, C, scale) IS the matrix (csr_rowptr, csr_col, csr_val): for every row the sorted union of its
 * P entries and of C (rows in S) or S (rows in C) equals the row's columns, every value equals scale[row] bit for bit, P is
 * symmetric, S and C are disjoint and J is not already part of P.  All pointers HOST pointers.  0 = proven, -1 = refuted
 * (a3vt_last_error says where). */
int a3vt_adj_split_validate(const int32_t *csr_rowptr, const int32_t *csr_col, const float *csr_val, int n_vert,
                            const int32_t *p_rowptr, const int32_t *p_col, const float *scale, const uint8_t *cls);

/* a3vt_gcn_stack_fwd / a3vt_gcn_stack_bwd_acc with the decomposition (`split` may be NULL: exactly the calls above).  The
 * backward must receive the split the forward received (the stash layout follows the forward's choice). */
int a3vt_gcn_stack_fwd_adj(const float *feats, int ld_feats, int in_features,
                           const float *const *weights, const float *const *biases,
                           int num_layers, int hidden, int cut_len,
                           const int32_t *csr_rowptr, const int32_t *csr_col, const float *csr_val, int csr_max_degree,
                           const a3vt_adj_split *split,
                           int n_vert, int batch, int gemm_bf16,
                           void *acts, uint8_t *masks, float *scratch, float *update, void *stream);
int a3vt_gcn_stack_bwd_adj(const float *feats, int ld_feats, int in_features,
                           const float *const *weights, const float *const *biases,
                           int num_layers, int hidden, int cut_len,
                           const int32_t *csr_rowptr, const int32_t *csr_col, const float *csr_val,
                           const int32_t *csrT_rowptr, const int32_t *csrT_col, const float *csrT_val, int csrT_max_degree,
                           const a3vt_adj_split *split,
                           int n_vert, int batch, int gemm_bf16,
                           const void *acts, const uint8_t *masks, const float *grad_update,
                           float *const *grad_weights, float *const *grad_biases, float *grad_feats,
                           float *scratch, int accumulate, void *stream);

/* One GCN layer on its own — GCN_layer.forward(features, adj, activation), model.py:351-363, for callers
 * that run their own layer loop (the copies in reconstruction/autoencoder/model.py:96-137 and
 * policies/DDQN/model.py:132-168 have layer shapes the stack entry points do not cover:
 * hidden -> hidden without the cut, hidden_dim -> num_actions).
 *   Z = X W ;  Y[:, :c] = A Z[:, :c] + b[:c] ;  Y[:, c:] = Z[:, c:] ;  Y = relu ? max(Y, 0) : Y
 * c = cut_len = round(out * cut) when the layer cuts (do_cut), c = out_features otherwise (all channels
 * aggregated, bias on all).  in_features <= ld_x <= 600, out_features <= 304.
 * x [M][ld_x] (ld_x % 4 == 0, pad columns zero), weight [in_features][out_features] (reference layout
 * (1,in,out)), bias [out_features], y [M][ld_y] (ld_y % 4 == 0, ld_y >= out_features; pad columns untouched).
 * Backward: grad_y [M][ld_gy] and the forward output y (the ReLU mask is y > 0) -> grad_x [M][ld_x] (pad
 * columns zero), grad_weight [in][out], grad_bias [out] (all overwritten; bias channels >= c get zeros). */
size_t a3vt_gcn_layer_scratch_bytes(int batch, int n_vert, int ld_x, int out_features, int cut_len,
                                    int need_backward);
int a3vt_gcn_layer_fwd(const float *x, int ld_x, int in_features, const float *weight, const float *bias,
                       int out_features, int cut_len, int relu,
                       const int32_t *csr_rowptr, const int32_t *csr_col, const float *csr_val, int csr_max_degree,
                       int n_vert, int batch, int gemm_bf16, float *y, int ld_y, float *scratch, void *stream);
int a3vt_gcn_layer_bwd(const float *x, int ld_x, int in_features, const float *weight,
                       int out_features, int cut_len, int relu,
                       const int32_t *csrT_rowptr, const int32_t *csrT_col, const float *csrT_val, int csrT_max_degree,
                       int n_vert, int batch, int gemm_bf16, const float *y, int ld_y, const float *grad_y, int ld_gy,
                       float *grad_weight, float *grad_bias, float *grad_x, float *scratch, void *stream);

/* The dense per-vertex product alone (torch.matmul(features, self.weight), model.py:352) on the
 * fp32 MFMA path: C[M][n_out] = A[M][k] * W[k][n_out], k % 4 == 0, n_out <= 304.  `wt` is W transposed
 * and zero padded to [a3vt_wt_rows(n_out)][a3vt_wt_ld(k)] floats (a3vt_transpose_weight builds it).
 * Used by tests and by bench.py to time the dominant kernel in isolation. */
int a3vt_wt_rows(int n_out);
int a3vt_wt_ld(int k);
int a3vt_transpose_weight(const float *w, int k, int n_out, float *wt, void *stream);
int a3vt_rowgemm(const float *a, int lda, int m, int k, const float *wt, int n_out, int gemm_bf16,
                 float *c, int ldc, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Vertex features.  Replaces Positional_Encoder.forward (model.py:381-399) + Mask_Encoder.forward
 * (model.py:410-414) + their sum (model.py:232,240,262,275):
 *   feats = MLP(nerf_embedding(p) ++ p) + Embedding[mask]
 * pe_params: packed fp32 [W1 (I/4 x 63), b1, W2 (I/2 x I/4), b2, W3 (I x I/2), b3, E (4 x I)],
 * each in torch (out,in) row-major layout (state-dict order).  Only I = 50 (the image-free model,
 * model.py:193) is supported by the fused kernel.  feats is [M][ld_feats], pad columns zeroed. */
size_t a3vt_posenc_param_count(int input_size);
size_t a3vt_posenc_scratch_bytes(int m, int input_size);
int a3vt_posenc_mask_fwd(const float *verts, const float *mask, int m, int input_size,
                         const float *pe_params, float *feats, int ld_feats, void *stream);
/* grad_params has a3vt_posenc_param_count floats (overwritten); grad_verts [M][3] (overwritten).
 * Row stride and alignment, both entries: any ld_feats >= input_size is accepted (a smaller one is refused), and feats /
 * grad_feats need no more than a float's alignment.  Columns input_size .. ld_feats - 1 of feats are written as zeros;
 * those of grad_feats are never used, whatever they hold.  The backward reads gradient rows in 16-byte pieces when
 * ld_feats % 4 == 0 and grad_feats is 16-byte aligned (52, the models' stride), and element by element otherwise
 * (ld_feats = 50 puts every odd row 8 bytes off): same result, the first is faster. */
int a3vt_posenc_mask_bwd(const float *verts, const float *mask, int m, int input_size,
                         const float *pe_params, const float *grad_feats, int ld_feats,
                         float *grad_verts, float *grad_params, float *scratch, void *stream);

/* The same encoder for wide inputs — input_size = 448 of the image models (model.py:180-190: 64 + 128 + 256 pooled channels)
 * — whose 133 k parameters do not fit the LDS-resident kernel above: every layer runs as one product on the fp32 matrix
 * pipe (csrc/posenc_wide.hip).  a3vt_posenc_wide_supported: input_size % 8 == 0, 16 <= input_size <= 496.  ld_feats must
 * equal input_size.  `acts` (a3vt_posenc_wide_acts_bytes) receives the layer activations in the forward and is read by the
 * backward — the caller keeps it between the two calls; `scratch` (a3vt_posenc_wide_scratch_bytes) is free afterwards.
 * pe_params / grad_params: the packing of a3vt_posenc_mask_fwd.  Replaces the same reference lines.
 * gemm_bf16: 0 = exact fp32 products (the default path), 1 = the products after the embedding layer, forward and
 * backward, take bf16-rounded operands (fp32 storage and accumulation; the bf16 configurations' knob). */
int a3vt_posenc_wide_supported(int input_size);
size_t a3vt_posenc_wide_acts_bytes(int m, int input_size);
size_t a3vt_posenc_wide_scratch_bytes(int m, int input_size, int need_backward);
int a3vt_posenc_wide_fwd(const float *verts, const float *mask, int m, int input_size, const float *pe_params,
                         float *feats, int ld_feats, float *acts, float *scratch, int gemm_bf16, void *stream);
int a3vt_posenc_wide_bwd(const float *verts, const float *mask, int m, int input_size, const float *pe_params,
                         const float *grad_feats, int ld_feats, const float *acts, float *grad_verts,
                         float *grad_params, float *scratch, int gemm_bf16, void *stream);

/* Per-vertex image features.  Replaces Image_Encoder.pooling (model.py:70-103): project the vertices with the fixed
 * camera matrix `proj` = K.RT (row-major 3 x 4, model.py:50-67; HOST pointer), z == 0 -> 0.1,
 * xs = P1/P2/256, ys = P0/P2/256, inf -> 0.5, then grid_sample(bilinear, zeros, align_corners=True) of every map at
 * (2 ys - 1, 2 xs - 1) and concatenation:  feats[b][v][off_k + c] for map k, channel c.
 * maps[k] is CHANNELS-LAST, [B][H_k][W_k][C_k] (torch channels_last memory of a (B,C,H,W) tensor), C_k % 4 == 0;
 * `maps`, `chans`, `heights`, `widths`, `grad_maps` are HOST arrays of n_maps (<= 4) entries.
 * feats / grad_feats are [B*N][ld_feats], ld_feats % 4 == 0, ld_feats >= sum C_k (other columns untouched).
 * Backward overwrites grad_maps[k] (same layout as maps[k]) and grad_verts [B*N][3] (the reference's autograd
 * reaches the vertex positions through the sampling grid; its in-place patches cut the gradient where they fire). */
int a3vt_image_pool_fwd(const float *verts, int batch, int n_vert, const float *proj_host, int n_maps,
                        const float *const *maps, const int *chans, const int *heights, const int *widths,
                        float *feats, int ld_feats, void *stream);
/* The same with the sum of model.py:243,265,277 folded in: feats = base + pooled, `base` = the positional + mask features
 * [B*N][ld_feats] (a3vt_posenc_mask_fwd); ld_feats must equal sum C_k.  One pass instead of the pooling's store plus a
 * separate 3 x 220 MB element-wise add per refinement stage of configs[3].  feats may not alias base. */
int a3vt_image_pool_fwd_add(const float *verts, int batch, int n_vert, const float *proj_host, int n_maps,
                            const float *const *maps, const int *chans, const int *heights, const int *widths,
                            const float *base, float *feats, int ld_feats, void *stream);
int a3vt_image_pool_bwd(const float *verts, int batch, int n_vert, const float *proj_host, int n_maps,
                        const float *const *maps, const int *chans, const int *heights, const int *widths,
                        const float *grad_feats, int ld_feats, float *const *grad_maps, float *grad_verts,
                        void *stream);

/* Bias gradient of a convolution whose output gradient is stored channels-last (the bias gradients of the nn.Conv2d
 * layers of the image pyramid, model.py:15-47, in the channels-last bf16 branch):
 *   out[c] = sum over rows of grad[row][c],  grad = [rows = N*H*W][channels] contiguous, fp32 (bf16 == 0) or bf16 (== 1),
 * 16-byte aligned; out fp32 [channels], overwritten.  Fixed summation order (repeatable bit for bit).
 * scratch: a3vt_bias_grad_scratch_bytes(rows, channels) bytes (0 = unsupported channel count). */
size_t a3vt_bias_grad_scratch_bytes(long long rows, int channels);
int a3vt_bias_grad_nhwc(const void *grad, int bf16, long long rows, int channels, float *out, void *scratch,
                        size_t scratch_bytes, void *stream);

/* Training-mode BatchNorm2d + ReLU of a `CNN_layer` (model.py:15-23: BatchNorm2d -> ReLU -> Conv2d; 13 per encoder and
 * step, model.py:147-164) on a channels-last bf16 map, three launches each way instead of 3 + 1 (+ the counter increment):
 *   y = relu(gamma * (x - mean_c) / sqrt(var_c + eps) + beta),  statistics over the rows per channel (biased variance);
 *   running_mean / running_var (unbiased variance, `momentum`) and *num_batches_tracked (+1) are updated as nn.BatchNorm2d
 *   does (pass NULL to skip either).  pre_bias (optional, fp32 [channels]): a per-channel constant the producer of x left
 *   out — the bias of the Conv2d in front: batch statistics remove any such shift, so y is the same without the 28 bias-add
 *   launches of a step, and only running_mean takes it (mean + pre_bias).  x, y, dy, dx: [rows = N*H*W][channels] bf16, 16-byte aligned; gamma, beta, dgamma,
 *   dbeta: fp32 [channels]; save: fp32 [4][channels] written by the forward (mean, 1/std, scale, shift), read by the backward.
 * Backward: dgamma = sum g * xhat, dbeta = sum g, dx = scale * (g - dbeta / rows - xhat * dgamma / rows), g = dy where y > 0
 * (the mask is recomputed from x with the forward's own coefficients).  dx_colsum (optional, fp32 [channels]): the column sums
 * of dx as stored in bf16 — when x is the output of a Conv2d this is that layer's bias gradient, which a3vt_bias_grad_nhwc would
 * otherwise compute by reading dx again.  Fixed summation order, float64 final sums: repeatable
 * bit for bit.  rows >= 2.  scratch: a3vt_bnrelu_scratch_bytes(channels) bytes; one buffer may serve every layer of a stream. */
size_t a3vt_bnrelu_scratch_bytes(int channels);
int a3vt_bnrelu_fwd(const void *x, long long rows, int channels, const float *gamma, const float *beta, const float *pre_bias,
                    float eps, float momentum, float *running_mean, float *running_var, long long *num_batches_tracked, void *y,
                    float *save, void *scratch, size_t scratch_bytes, void *stream);
int a3vt_bnrelu_bwd(const void *dy, const void *x, long long rows, int channels, const float *save, void *dx, float *dgamma,
                    float *dbeta, float *dx_colsum, void *scratch, size_t scratch_bytes, void *stream);

/* bf16 copies of the pyramid's fp32 convolution weights and biases (the nn.Conv2d parameters of model.py:15-47) for MIOpen's
 * NHWC bf16 kernels, all in one launch per optimizer step instead of two or three per tensor: tensor k is
 * src[k] fp32 [outer[k]][inner[k]][hw[k]] (a weight: O x I x (KH KW), contiguous; a bias: inner = hw = 1) and becomes
 * dst[k] bf16 [outer][hw][inner] (channels-last), round to nearest even.  n <= 96; the five arrays are HOST arrays of n
 * entries holding device pointers / sizes. */
int a3vt_cast_weights_bf16(int n, const float *const *src, void *const *dst, const long long *outer, const int *inner,
                           const int *hw, void *stream);

/* The 5 x 5 convolutions of the image pyramid's small-channel layers (`CNN_layer`'s nn.Conv2d(kernel_size = 5, padding = 1),
 * model.py:15-47) on channels-last bf16 maps, which MIOpen runs at a tenth of the rate their bytes allow.  Shapes taken
 * (a3vt_conv5_supported): (cin, cout, stride) = (16, 16, 1), (32, 32, 1) — layers 2-3 and 5-6 of Image_Encoder —, (16, 32, 2),
 * layer 4, and the 3-channel layers 0 and 1: (3, 3, 1) and (3, 16, 2), forward only (flip = 0).   y[b][oy][ox][co] = bias[co] + sum over (ky, kx, ci) of x[b][oy stride + ky - pad][ox stride + kx - pad][ci] * Wm[co][ky][kx][ci]
 * (pixels outside the map are zeros); x: [batch][height][width][cin] bf16, y: [batch][Ho][Wo][cout] bf16 with
 * Ho = (height + 2 pad - 5) / stride + 1; fp32 accumulation, one rounding.  `image` (a3vt_conv5_image_bytes bytes, 16-byte
 * aligned) is written by a3vt_conv5_weight_image from the fp32 weight [cout][cin][5][5] (OIHW): flip = 0 with pad = 1 is the
 * layer's forward; for the stride-1 shapes flip = 1 (Wm transposed and flipped: call the convolution with cin and cout swapped)
 * with pad = 3 applied to the OUTPUT gradient is the gradient with respect to the layer's input.  bias: fp32 [cout] or NULL.
 * (Weight gradients, and the input gradient of the stride-2 layer, stay on MIOpen.) */
int a3vt_conv5_supported(int cin, int cout, int stride);
size_t a3vt_conv5_image_bytes(int cout, int cin, int flip);
int a3vt_conv5_weight_image(const float *weight, int cout, int cin, int flip, void *image, void *stream);
int a3vt_conv5_nhwc(const void *x, int batch, int height, int width, int cin, int cout, int stride, int pad, const void *image,
                    const float *bias, void *y, void *stream);

/* The input gradient of the pyramid's layer 1 (nn.Conv2d(3, 16, 5, stride 2, padding 1)): grad_out [batch][out_height][out_width][16]
 * bf16 -> grad_in [batch][2 out_height + 2][2 out_width + 2][3] bf16 (= the layer's input size when (H + 2 - 5) is odd, as for the
 * 254-pixel map), computed as the stride-1 convolution of a3vt_conv5_nhwc on grad_out read as if upsampled by two with zeros;
 * `image` = a3vt_conv5_weight_image(weight [16][3][5][5], cout 16, cin 3, flip 1). */
int a3vt_conv5_input_grad_3x16s2(const void *grad_out, int batch, int out_height, int out_width, const void *image, void *grad_in,
                                 void *stream);

/* The weight gradient of the same five layers ((cin, cout, stride) = (3, 3, 1), (3, 16, 2), (16, 16, 1), (32, 32, 1), (16, 32, 2);
 * padding 1) — autograd's third product of nn.Conv2d at vision/model.py:15-23:
 *   grad_weight[co][ci][ky][kx] = sum over (b, oy, ox) of grad_out[b][oy][ox][co] * x[b][oy stride + ky - 1][ox stride + kx - 1][ci],
 * x: [batch][height][width][cin] bf16 (the layer's input), grad_out: [batch][Ho][Wo][cout] bf16, grad_weight: fp32 [cout][cin][5][5]
 * (OIHW), overwritten.  fp32 accumulation on the matrix pipe, partial sums per workgroup added in a fixed order (repeatable bit
 * for bit; MIOpen's kernel accumulates with atomics into an fp32 workspace it first fills and then casts).  scratch:
 * a3vt_conv5_wrw_scratch_bytes(cin, cout) bytes, 16-byte aligned; x / grad_out 16-byte aligned for 16 / 32 channels, 2-byte for 3. */
size_t a3vt_conv5_wrw_scratch_bytes(int cin, int cout);
int a3vt_conv5_weight_grad(const void *x, const void *grad_out, int batch, int height, int width, int cin, int cout, int stride,
                           float *grad_weight, void *scratch, size_t scratch_bytes, void *stream);

/* The fp32 5 x 5 convolutions of the touch chart predictor's stem (`DoubleConv` blocks 1-3 of `Encoder`, reconstruction/touch/
 * model.py:10-47) on channels-last fp32 maps, with the per-channel affine map of an eval-mode BatchNorm and the ReLU in the epilogue:
 *   y[b][oy][ox][co] = act(scale[co] * (sum over (ky, kx, ci) of x[b][oy stride + ky - pad][ox stride + kx - pad][ci] * W[co][ci][ky][kx]) + shift[co])
 * (pixels outside the map are zeros; act = max(., 0) with relu = 1, the identity with relu = 0; scale / shift: fp32 [cout], NULL = 1 / 0).
 * x: [batch][height][width][cin] fp32, y: [batch][Ho][Wo][cout] fp32, Ho = (height + 2 pad - 5) / stride + 1, pad in 0 .. 4.
 * Shapes taken (a3vt_conv5f_supported): (cin, cout, stride) = (3, 16, 2), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 32, 2).
 * Exact fp32 on the matrix pipe (v_mfma_f32_16x16x4_f32: a chain of fused multiply-adds); every output element is ONE chain over
 * (tap, channel) in a fixed order, so a result depends neither on the batch around it nor on the launch: repeatable bit for bit.
 * `image` (a3vt_conv5f_image_bytes(cin, cout) bytes; 0 for channel counts not taken) is written by a3vt_conv5f_weight_image from the
 * fp32 weight [cout][cin][5][5] (OIHW).  image and y 16-byte aligned; x 16-byte aligned for 16 / 32 channels, 4-byte for 3.  No
 * allocation, no host synchronisation; invalid arguments (NULL pointers, a shape not taken, batch < 1, pad outside 0 .. 4, an empty
 * output) return < 0 before anything is launched.  Forward only. */
int a3vt_conv5f_supported(int cin, int cout, int stride);
size_t a3vt_conv5f_image_bytes(int cin, int cout);
int a3vt_conv5f_weight_image(const float *weight, int cout, int cin, void *image, void *stream);
int a3vt_conv5f_nhwc(const float *x, int batch, int height, int width, int cin, int cout, int stride, int pad, const void *image,
                     const float *scale, const float *shift, int relu, float *y, void *stream);

/* The optimizer step of the trainer, `optim.Adam(params, lr, weight_decay=0)` + `optimizer.step()` (vision/train.py:64,148), over ALL
 * parameter tensors in one launch — torch's Adam (amsgrad off, maximize off) in its own order of operations per element:
 *   g' = g + weight_decay p;  m += (g' - m)(1 - beta1);  v = v beta2 + ((1 - beta2) g') g';
 *   p -= lr / (1 - beta1^step) * (m / (sqrt(v) / sqrt(1 - beta2^step) + eps)),      step = 1 for the first call.
 * The tensors (fp32, contiguous, any alignment; 16-byte aligned ones take the vector path) are described by DEVICE tables the caller
 * builds once: param / grad / exp_avg / exp_avg_sq [tensors] pointers, numel [tensors], and a chunk list — chunk k covers elements
 * [chunk_off[k], chunk_off[k] + a3vt_adam_chunk_elems()) of tensor chunk_tensor[k] (cut off at numel); every element must be covered
 * exactly once.  Element-wise and without reductions: bit-repeatable. */
int a3vt_adam_chunk_elems(void);
int a3vt_adam_step(void *const *param, const void *const *grad, void *const *exp_avg, void *const *exp_avg_sq,
                   const long long *numel, const int *chunk_tensor, const long long *chunk_off, int n_chunks, double lr, double beta1,
                   double beta2, double eps, double weight_decay, long long step, void *stream);
/* The same step with the reference learner's gradient clamp in front of it (policies/DDQN/ddqn.py:120-122, `param.grad.data.clamp_(-1, 1)`)
 * inside the same launch: every gradient element is clamped to [-grad_clamp, grad_clamp] (grad_clamp > 0), the clamped value is what
 * the step uses AND what is left in the gradient tensor, as the in-place clamp leaves it. */
int a3vt_adam_step_clamp(void *const *param, void *const *grad, void *const *exp_avg, void *const *exp_avg_sq, const long long *numel,
                         const int *chunk_tensor, const long long *chunk_off, int n_chunks, double lr, double beta1, double beta2,
                         double eps, double weight_decay, long long step, double grad_clamp, void *stream);

/* Vertex update, model.py:250,270,283:  out[b][v] = in[b][v] + (v < n_vision ? update[b][v] : 0). */
int a3vt_vertex_update(const float *verts_in, const float *update, int batch, int n_vert, int n_vision,
                       float *verts_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Surface sampling.  Replaces batch_sample, utility/utils.py:152-187 (PyTorch3D
 * mesh_face_areas_normals + torch.multinomial + _rand_barycentric_coords + gathers).
 * faces [F][3] int32 is shared by the whole batch (adj_info['faces']).
 * a3vt_face_cdf: per-mesh inclusive CDF of p_f = |area_f / sum(area)| with the reference's NaN
 * scrubs (utils.py:165-168): cdf [batch][F].
 * a3vt_sample_points_fwd: `draws` independent clouds of `num` points per mesh (utils.chamfer_distance
 * draws 3, utils.py:204-217).  If face_idx_in/u_in/v_in are non-NULL ([draws][batch][num]) they are
 * used as the samples (parity mode); otherwise samples come from Philox4x32-10(seed, offset) through
 * the CDF.  Outputs: points [draws][batch][num][3] and the samples actually used (face_idx/u/v out,
 * needed by the backward pass). */
int a3vt_face_cdf(const float *verts, const int32_t *faces, int batch, int n_vert, int n_faces,
                  float *cdf, void *stream);
int a3vt_sample_points_fwd(const float *verts, const int32_t *faces, const float *cdf,
                           int batch, int n_vert, int n_faces, int draws, int num,
                           const int32_t *face_idx_in, const float *u_in, const float *v_in,
                           uint64_t seed, uint64_t offset,
                           float *points, int32_t *face_idx_out, float *u_out, float *v_out, void *stream);
/* grad_verts [batch][n_vert][3] is overwritten with the scatter-add of w_k * grad_points. */
int a3vt_sample_points_bwd(const int32_t *faces, int batch, int n_vert, int n_faces, int draws, int num,
                           const int32_t *face_idx, const float *u, const float *v,
                           const float *grad_points, float *grad_verts, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Chamfer.  Replaces pytorch3d.loss.chamfer_distance(x, y, batch_reduction=None) as called at
 * utility/utils.py:207,212 (squared-L2 K=1 nearest neighbour both ways, mean over each cloud, summed)
 * and the mean over draws at utils.py:214-215.
 * x [draws][batch][p][3] (predicted clouds), y [batch][q][3] (ground truth, shared by the draws).
 * Outputs: dist_xy/idx_xy [draws][batch][p], dist_yx/idx_yx [draws][batch][q],
 *          cd [batch] = (1/draws) sum_r ( mean_i dist_xy + mean_j dist_yx ).
 * scratch: a3vt_chamfer_scratch_bytes() bytes (8 per ground-truth point and cloud), contents irrelevant: with it both
 *          directions come out of ONE pass over the distance matrix; NULL selects the two-pass search (same results,
 *          bit for bit — every distance is the same fma chain and ties go to the lowest index either way). */
size_t a3vt_chamfer_scratch_bytes(int draws, int batch, int p, int q);
int a3vt_chamfer_fwd(const float *x, const float *y, int draws, int batch, int p, int q,
                     float *dist_xy, int32_t *idx_xy, float *dist_yx, int32_t *idx_yx, float *cd,
                     void *scratch, void *stream);
/* The same with a sized workspace and a choice of search.  a3vt_chamfer_workspace_bytes() holds every algorithm.
 * algo: 0 = automatic (the pruned search from 2048 points per cloud on, else the sweep), 1 = brute force, one launch
 *       per direction (workspace may be NULL), 2 = brute force, one sweep, 3 = pruned exact search: each cloud is
 *       sorted into blocks of 64 neighbouring points with bounding boxes, and a wave of 64 neighbouring queries only
 *       evaluates the blocks whose box can still hold a nearer (or equally near) point.
 * All algorithms return the same distances and indices bit for bit (same fma chain, ties to the lowest index).
 * <0 if the workspace is too small for the algorithm asked for (or, for the pruned search, not 16-byte aligned). */
size_t a3vt_chamfer_workspace_bytes(int draws, int batch, int p, int q);
int a3vt_chamfer_fwd_ws(const float *x, const float *y, int draws, int batch, int p, int q,
                        float *dist_xy, int32_t *idx_xy, float *dist_yx, int32_t *idx_yx, float *cd,
                        void *workspace, size_t workspace_bytes, int algo, void *stream);
/* Forward-only callers that score K candidate meshes per ground-truth cloud (policies/environment.py:174-180,252-257: the
 * greedy search evaluates up to 50 candidate touches against the same object): y holds y_batch clouds, batch is a multiple
 * of y_batch and mesh b is compared with y[b % y_batch] — the ground truth is uploaded, sorted and boxed once instead of
 * once per candidate.  Outputs as a3vt_chamfer_fwd_ws (dist_yx / idx_yx per mesh: [draws][batch][q]). */
int a3vt_chamfer_fwd_shared(const float *x, const float *y, int draws, int batch, int y_batch, int p, int q,
                            float *dist_xy, int32_t *idx_xy, float *dist_yx, int32_t *idx_yx, float *cd,
                            void *workspace, size_t workspace_bytes, int algo, void *stream);
/* grad_cd [batch].  grad_x [draws][batch][p][3] overwritten; grad_y [batch][q][3] overwritten, may be
 * NULL (the trainer's ground truth needs no gradient, vision/train.py:141-143).  Every index must be in range.
 * A NaN or Inf coordinate makes the gradient of every cloud it enters NaN throughout: x[r][b] poisons grad_x[r][b] and
 * grad_y[b], y[b] poisons grad_x[.][b] and grad_y[b]; the other clouds are unaffected. */
int a3vt_chamfer_bwd(const float *x, const float *y, int draws, int batch, int p, int q,
                     const int32_t *idx_xy, const int32_t *idx_yx, const float *grad_cd,
                     float *grad_x, float *grad_y, void *stream);

/* Test hook (tests/test_gpu_csr_sliced.py): which neighbour-aggregation kernels the fp32 stacks use — 0 = chosen by shape
 * (default), 1 = the half-wave-per-vertex kernels everywhere, 2 = the channel-sliced kernels wherever a mesh slice fits
 * LDS, graphs with long rows included.  In the bf16 storage mode 1 also keeps the row walk where the tiled aggregation
 * (neighbour rows from LDS, bit-identical sums) would run.  Every choice gives the same outputs; process-wide; not a tuning
 * knob.  The library reads NO environment variable. */
int a3vt_dbg_csr_algo(int algo);

/* Test hook: how many launch decisions of this process took each kernel family since the last reset — so that a parity test
 * can assert that its fixture REACHES the kernels it claims to pin (tests/test_gpu_golden.py::test_g12_*).  counts[0..n):
 *   [0] stack forward calls on the channel-sliced aggregation (hybrid rows)   [1] ... on the half-wave row-walk kernels
 *   [2] rowgemm_kernel<19,...,ADIRECT> launches (exact fp32 hidden-layer products: the headline kernel)
 *   [3] rowgemm3_kernel launches (gemm mode 3)   [4] dw3_kernel launches   [5] dw_kernel launches on quad-major operands
 *   [6] rowgemm16_kernel launches (bf16 storage)  [7] bf16-storage stack forward calls on the channel-sliced aggregation
 *   [8] rowgemmw_kernel launches  [9] dww_kernel launches (exact fp32 hidden-layer products, round 6)
 *   [10] stack forward calls that aggregated through the P + bipartite split (struct a3vt_adj_split)
 *   [11] csr16t forward launches (bf16 storage: aggregation from LDS tiles)
 *   [12] a3vt_qnet_input_fwd calls  [13] a3vt_qnet_input_bwd calls  [14] a3vt_fold_fwd calls  [15] a3vt_fold_bwd calls
 *   [16] csr3s_kernel launches (the 3-channel output-layer aggregation through the split, forward or transposed)
 * Returns the number of counters the library keeps (entries beyond it are written as 0); reset != 0 clears them. */
int a3vt_dbg_path_counts(long long *counts, int n, int reset);

/* Test hook: WORK counters of the pruned nearest-neighbour search (a3vt_chamfer_fwd_ws and friends) — values cannot show a
 * search that does too much work (round 5: pad lanes that asked about the origin cost 1.85 ms of a 1.5 ms launch for three
 * rounds, every result bit-exact).  enable != 0 clears the counters and switches them on for the searches that follow (a
 * handful of atomics per wave: not for timing), enable == 0 switches them off; out8 != NULL receives what was counted so
 * far: [0] waves of 64 queries, [1] groups of 16 candidates evaluated, [2] blocks of 64 evaluated, [3] point-to-box tests,
 * [4] the most groups any one wave evaluated, [5..7] 0.  Synchronises the device.  Off by default (the product touches no
 * counter). */
int a3vt_dbg_nn_work(int enable, unsigned long long *out8);

/* The operand split of gemm mode 3 (replaces nothing in the reference: it is how torch.matmul(features, self.weight),
 * model.py:352, is fed to the bf16 matrix pipe without losing fp32 bits).  hi / mid / lo receive bf16 bit patterns with
 * float(hi[i]) + float(mid[i]) + float(lo[i]) == x[i] exactly for every finite x[i] whose lowest set bit is >= 2^-133
 * (all normal floats down to 2^-110; FLT_MAX included: hi is a truncation and cannot overflow); smaller magnitudes
 * differ by < 2^-133.  Device pointers, n elements each. */
int a3vt_split3_bf16(const float *x, size_t n, uint16_t *hi, uint16_t *mid, uint16_t *lo, void *stream);

/* ---------------------------------------------------------------------------------------------
 * One FoldingNet fold of the auto-encoder's decoder (reconstruction/autoencoder/model.py: FoldingNetDecFold1 / Fold2,
 * conv3(relu(conv2(relu(conv1(cat(code, g))))))) over batch * points rows, without any (batch * points) x 512 tensor in
 * memory.  conv1 of the concatenated input is split by the caller: bias_s (batch, 512) = W1[:, :512] code_b + b1, and
 * w1g (512, k) = W1[:, 512:], k = 2 (fold 1: the lattice) or 3 (fold 2: fold 1's output).  g (batch, points, k),
 * w2 (512, 512), b2 (512), w3 (3, 512), b3 (3), y / dy (batch, points, 3): all fp32, row-major, device pointers.
 * Exact fp32 (v_mfma_f32_32x32x2_f32); every sum over rows has a fixed order, so two calls give the same bits, and a
 * sample's forward does not depend on the batch around it.  width is the layer width and must be 512 (the compiled
 * shape).  bias_s, w2, b2, w3, dw2 and the workspace are 16-byte aligned.  The workspace (a3vt_fold_workspace_bytes;
 * backward != 0 for a3vt_fold_bwd) holds the operand images of w2, the sign bits of the second activation (64 bytes per
 * row) and the partial sums; nothing in it survives a call.
 * a3vt_fold_bwd: d_bias_s (batch, 512), dg (batch, points, 3; NULL when k = 2 or not wanted), dw1g (512, k),
 * dw2, db2, dw3, db3 are overwritten.  Returns 0, or non-zero with a message in a3vt_last_error. */
size_t a3vt_fold_workspace_bytes(int batch, int points, int backward);
int a3vt_fold_fwd(const float *bias_s, const float *g, int k, const float *w1g, const float *w2, const float *b2, const float *w3,
                  const float *b3, int batch, int points, int width, float *y, void *workspace, size_t workspace_bytes, void *stream);
int a3vt_fold_bwd(const float *bias_s, const float *g, int k, const float *w1g, const float *w2, const float *b2, const float *w3,
                  const float *dy, int batch, int points, int width, float *d_bias_s, float *dg, float *dw1g, float *dw2, float *db2,
                  float *dw3, float *db3, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The double-DQN learner (policies/DDQN/ddqn.py:81-125).
 *
 * a3vt_ddqn_td: target, loss and what the loss gradient needs in one launch, from the three Q-network outputs of an update.
 * q_cur, q_next_online, q_next_target, mask: [batch][num_actions] fp32; actions [batch] fp32 (the replay memory stores them as
 * floats; values outside [0, num_actions) are clamped into it); rewards [batch]; denom [batch] or NULL (rewards / denom: the
 * reference's "first" / "current" normalisation).  Per sample: not_done = sum(mask) < budget - 1 (the CURRENT mask, as the
 * reference); best_next = argmax of q_next_online with -1e10 where mask > 0, the lowest index on a tie;
 * target = gamma * (not_done ? q_next_target[best_next] : 0) + reward; diff = q_cur[action] - target; loss[0] = mean(diff^2),
 * summed in a fixed order (no atomics: the same bits on every call).  batch <= 4096, num_actions <= 304; anything else is
 * an argument error.  No host sync.
 * a3vt_ddqn_td_bwd: dq_cur[b][a] = grad_loss[0] * 2 * diff[b] / batch at a = actions[b], 0 elsewhere (grad_loss: device). */
int a3vt_ddqn_td(const float *q_cur, const float *q_next_online, const float *q_next_target, const float *mask, const float *actions,
                 const float *rewards, const float *denom, int batch, int num_actions, int budget, float gamma, float *loss,
                 float *diff, int32_t *best_next, float *target, void *stream);
int a3vt_ddqn_td_bwd(const float *diff, const float *actions, const float *grad_loss, int batch, int num_actions, float *dq_cur,
                     void *stream);

/* ---------------------------------------------------------------------------------------------
 * The nearest-neighbour latent policy's bank lookup (policies/NearestNeighbor/train.py:114-137).
 *
 * a3vt_latent_nearest: for each of n_queries latents the k nearest rows of a bank, and the action of the first of them that has not
 * been taken.  bank [bank_rows][dim] fp32, contiguous; queries [n_queries][dim]; taken [n_queries][num_actions] fp32, non-zero = the
 * action was already performed (the environment's obs["mask"] as it is), NULL excludes nothing; bank_actions [bank_rows] int32, NULL
 * only together with action and rank (a pure k-nearest query).
 * Distance: d(e, j) = (1 / dim) * sum_c (bank[j][c] - queries[e][c])^2 in fp32.  The order of operations of one (query, row) pair is
 * fixed and depends neither on the row's position, bank_rows, n_queries nor the query's position: bit-identical rows have
 * bit-identical distances, and a query's results do not change bit-wise when other queries or farther rows are added.
 * Outputs: idx, dist [n_queries][k] hold the k_eff = min(k, bank_rows) nearest rows, nearest first; a tie goes to the LOWER row
 * index; a NaN distance ranks after every number, +inf included (as torch.topk(largest=False) ranks it); entries from k_eff on are
 * -1 and +inf.  action[e] = bank_actions of the first listed row whose action a lies in [0, num_actions) and has taken[e][a] == 0,
 * rank[e] its position in the list; both -1 when no listed row qualifies.  A bank action outside the range never qualifies and
 * never indexes taken.
 * Limits: 1 <= dim <= 4096, 1 <= n_queries <= 1024, 1 <= k <= 64, 1 <= bank_rows <= 2^24, 1 <= num_actions <= 304.  Anything else,
 * a null required pointer, a null scratch (a3vt_latent_nearest_scratch_bytes bytes; 0 for unsupported sizes) or a misaligned pointer
 * (bank and queries: 16 bytes when dim % 4 == 0; everything else 4) returns non-zero with a message in a3vt_last_error and launches
 * nothing.  Two kernel launches on `stream`; no host synchronisation, no allocation, no float atomics: the same bits on every call.
 * A bank of more than a3vt_latent_nn_cached_rows() rows is selected from the scratch rather than from registers: a thread whose key
 * was taken reads its share of the query's distances again.  a3vt_latent_nn_tile(): bank rows per workgroup; a3vt_latent_nn_query_floats(): floats of queries held in
 * LDS at a time (queries are processed in chunks of that / dim). */
size_t a3vt_latent_nearest_scratch_bytes(int n_queries, int bank_rows, int k);
int a3vt_latent_nearest(const float *bank, const int32_t *bank_actions, int bank_rows, int dim, const float *queries, const float *taken,
                        int n_queries, int num_actions, int k, int32_t *idx, float *dist, int32_t *action, int32_t *rank, void *scratch,
                        void *stream);
int a3vt_latent_nn_tile(void);
int a3vt_latent_nn_query_floats(void);
int a3vt_latent_nn_cached_rows(void);

/* ---------------------------------------------------------------------------------------------
 * The dataset-specific policies' bookkeeping on one (K, E) score table (policies/dataset_specific/LEBA.py:115-128, MFBA.py:95-99).
 *
 * a3vt_candidate_tally makes one launch on `stream`.  It does no allocation, no host synchronisation and no atomics, and gives the
 * same bits on every call.
 *   scores      [K][E]
 *   candidates  [K][E]: the action candidate k tries on element e
 *   first_score [E], or NULL when sums is NULL
 *   taken       [E][A] fp32, non-zero = performed (obs["mask"] as it is); NULL excludes nothing
 *   unvisited   LEBA's sentinel, 1e10
 *   sums, checks [A] in/out, both or neither
 *   votes       [A] in/out or NULL
 *   best, best_score [E] out; best required when votes is given
 *
 * Greedy choice.
 * - best[e] is candidates[k][e] of the lowest scores[k][e] over k ascending.
 * - Only pairs with taken == NULL or taken[e][a] == 0 are eligible.
 * - A tie goes to the lower k.
 * - A NaN ranks after +inf.  This is the ordering rule of a3vt_latent_nearest and a3vt_latent_policy_fwd.
 * - The results are -1 and +inf when no pair is eligible.
 * - For tables without NaN this is environment.choose_actions.
 *
 * LEBA tally (reference LEBA.py:115-128).
 * - It runs for k ascending and, within k, e ascending, with a = candidates[k][e].
 * - r = scores[k][e] / first_score[e] is one correctly rounded fp32 division (__fdiv_rn in the kernel; no compiler flag decides it).
 * - If sums[a] == unvisited, compared in double, then sums[a] = (double)r.
 * - Otherwise sums[a] = (double)((float)sums[a] + r).
 * - The running sum is rounded to fp32 at every add and stored as a double.  That is what the reference computes: NumPy's
 *   float64 scalar + a 0-d fp32 torch tensor defers to torch and returns an fp32 tensor.
 * - checks[a] += 1.0 in double.
 * - The taken mask plays no part in the tally.
 *
 * MFBA votes (MFBA.py:98-99).
 * - For e ascending: votes[best[e]] += 1.0 in double when best[e] >= 0.
 *
 * Shared rules.
 * - A candidate outside [0, A) is skipped by every rule and never indexes taken, sums, checks or votes.  The Python layer refuses
 *   such a table.
 * - All updates of one action happen in the stated order whatever the launch geometry.
 *
 * Limits.
 * - 1 <= K <= 304.
 * - 1 <= E <= 1024.
 * - 1 <= A <= 304.
 * - Pointers are 4-byte aligned, the doubles 8-byte aligned.
 * - Anything else, or a missing required pointer, returns non-zero with a message in a3vt_last_error that names the argument and
 *   its value.  Nothing is launched. */
int a3vt_candidate_tally(const float *scores, const int32_t *candidates, const float *first_score, const float *taken, int K, int E, int A,
                         double unvisited, double *sums, double *checks, double *votes, int32_t *best, float *best_score, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The candidate inputs of one greedy step from the per-episode touch table (policies/environment.py:score_candidates, get_inputs).
 *
 * A touch does not depend on what was touched before, so ActiveTouch computes the chart and code of every (element, action,
 * finger) once per episode.  a3vt_touch_assemble writes the touch charts and masks of K candidate action lists over E elements
 * in the layout the reconstructor takes, candidate-major.
 *   table_charts [E][A][F][C][3]   the chart action a would put on finger f of element e
 *   table_codes  [E][A][F] int32   2 = "touch", 1 = "no_touch", 0 = no contact
 *   state_charts [E][F][G][C][3], state_masks [E][F][G][C]   the episode's touch state: G grasp slots of C chart vertices
 *   candidates   [K][E] int32      the action candidate k tries on element e
 *   slot                           the grasp slot the candidates fill
 *   charts       [K][E][F][G][C][3] out, masks [K][E][F][G][C] out
 *
 * Output rules.
 * - For g != slot, block (k, e, f, g) of both outputs is a copy of the state's block (e, f, g).
 * - For g == slot, with a = candidates[k][e]: charts[k][e][f][slot] = table_charts[e][a][f], and every value of
 *   masks[k][e][f][slot] is (float) of table_codes[e][a][f] clamped into 0..2.
 * - An action outside [0, A) gives a zero chart and mask 0 in that block.  It never indexes the table.  (The Python layer refuses
 *   such a list when it has it on the host.)
 * - Every value moves as 32 bits unchanged: NaN payloads, infinities and -0 survive.
 * - No input is written.  The outputs must not overlap the inputs.
 *
 * One launch on `stream`.  No allocation, no host synchronisation, no atomics, no workspace, no environment variable: the same
 * bits on every call.
 *
 * Limits.
 * - K, E, A, F, G, C >= 1 and 0 <= slot < G.
 * - K * E * F * G * C * 3 < 2^31.
 * - Every pointer is required and 4-byte aligned; no wider alignment is assumed (a block of C = 25 vertices is 300 bytes).
 * - Anything else returns non-zero with a message in a3vt_last_error that names the argument and its value.  Nothing is launched.
 *
 * a3vt_touch_assemble_launches: [0] the a3vt_touch_assemble calls that launched since the last reset; returns 1. */
int a3vt_touch_assemble(const float *table_charts, const int32_t *table_codes, const float *state_charts, const float *state_masks,
                        const int32_t *candidates, int K, int E, int A, int F, int G, int C, int slot, float *charts, float *masks,
                        void *stream);
int a3vt_touch_assemble_launches(long long *counts /*[1]*/, int reset);

/* ---------------------------------------------------------------------------------------------
 * The head of the touch chart predictor (reconstruction/touch/model.py: Encoder.fc, the template add, transform_verts) and the slot
 * rule of policies/scoring.py:touch_slots, for n views in one launch.
 *   features [n][512]            what the encoder's convolutions leave per view
 *   w1 [256][512], b1 [256]      fc.0.0, as torch stores a Linear: weight [out][in]
 *   w2 [128][256], b2 [128]      fc.1.0
 *   w3 [75][128],  b3 [75]       fc.2.0
 *   tmpl [25][3]                 the chart template
 *   rot [n][3][3], pos [n][3]    the finger frames
 *   code [n] int32               2 = "touch", 1 = "no_touch", anything else = no contact
 *   rows   [n][25][4] out        x, y, z, mask: the layout of a data set's touch_charts.npy
 *   charts [n][25][3], masks [n][25] out, both or neither (NULL): the same values as touch_slots' two tensors
 *
 * Per view: v = tmpl + fc(features) as 25 x 3, with ReLU after the first two layers (a NaN stays a NaN); w = rot . v + pos
 * (w[p][a] = ((rot[a][0] v[p][0] + rot[a][1] v[p][1]) + rot[a][2] v[p][2]) + pos[a], one rounding per multiply-add, then the add).
 *   code 2: w, mask 2.    code 1: pos in all 25 rows, mask 1.    otherwise: zeros, mask 0.
 * The rule is a select: no value of a view whose code is not 2 comes from its features or rot, and with any code but 1 and 2 none
 * comes from pos, so a NaN there does not reach the outputs.  No view's output depends on another view.
 *
 * Exact fp32.  The order of every sum is fixed and does not depend on n or on the view's index (csrc/chart_head.hip states it): the
 * same view gives the same bits alone, inside any batch and at any position.  One launch on `stream`.  No allocation, no host
 * synchronisation, no atomics, no workspace, no environment variable.  No input is written; outputs must not overlap inputs.
 *
 * Limits.
 * - n >= 1 and n * 512 < 2^31.
 * - features, w1, w2, w3 and rows are 16-byte aligned, every other pointer 4-byte aligned; all are required except charts and
 *   masks, which come together.
 * - Anything else returns non-zero with a message in a3vt_last_error that names touch_chart_head, the argument and its value.
 *   Nothing is launched.
 *
 * a3vt_touch_chart_head_launches: [0] the a3vt_touch_chart_head calls that launched since the last reset; returns 1. */
int a3vt_touch_chart_head(const float *features, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                          const float *b3, const float *tmpl, const float *rot, const float *pos, const int32_t *code, int n, float *rows,
                          float *charts, float *masks, void *stream);
int a3vt_touch_chart_head_launches(long long *counts /*[1]*/, int reset);

/* ---------------------------------------------------------------------------------------------
 * The rendered touch sampler: from finger frames and triangles to every signal of simulator/scene/instance.py:121-258.
 *
 * A batch of I finger views over a table of M meshes.
 *   verts       [V][3] fp32, the meshes' vertices concatenated
 *   faces       [F][3] int32, indices into verts (already global), as stored: no duplicated or flipped copies are needed
 *   face_offset [M + 1] int32: mesh m owns faces face_offset[m] .. face_offset[m + 1] - 1
 *   image_mesh  [I] int32: the mesh view i looks at
 *   cam_pos     [I][3], cam_rot [I][3][3]: the finger frame {"pos", "rot"} as the dataset's *_ref_frame.npy stores it
 *   max_depth, yfov (radians), znear, zfar: the reference's 0.025, 40 degrees, 1e-4, 10
 *   depth       [I][121][121] out
 *   touch       [I][121][121][3] out, or NULL
 *   points      [I][14641][3] out with count [I] int32 out: both or neither.  Rows from count[i] on are not written.
 *   status      [I] int32 out: 1 = "touch", 0 = "no_touch"
 *
 * Depth (a3vt_touch_render's first launch).
 * - The camera rotation is C = cam_rot . R_y(-90 deg) (instance.py:127-133): the camera looks along the finger's +x.
 * - It is a pinhole at cam_pos looking down its -z.  Pixel (r, c), row 0 at the top, has the centre x = (c + 0.5) / 121 * 2 - 1,
 *   y = 1 - (r + 0.5) / 121 * 2 and the ray (x tan(yfov / 2), y tan(yfov / 2), -1) in the eye frame.
 * - depth[r][c] is the ray parameter (= -z in the eye frame) of the nearest triangle hit with znear <= depth <= zfar; 0 without one.
 * - Casting is two-sided and inclusive on edges.  Across an edge that two faces share BY VERTEX INDEX it is watertight: no ray
 *   passes between them.
 * - This is ray casting at pixel centres.  It has not been compared with pyrender's rasteriser.
 *
 * Finish (the second launch; a3vt_touch_finish is that launch alone on depth maps the caller supplies).
 * - Every comparison of a depth with max_depth is an fp32 comparison, as NumPy makes it for a float32 map.
 * - status is 1 iff #(depth <= max_depth) - #(depth == 0) > 0 (instance.py:142).
 * - touch is depth_to_touch (:207-258) in fp32: pixels with depth > max_depth or == 0 become 1; gel = -(d - max_depth), 0 where
 *   d >= max_depth, then * 6 / max_depth / 30 + 0.4; the 7 x 7 mean with the boundary d c b a | a b c d of the map before any
 *   write-back replaces the zeroed pixels; np.gradient (central differences, one-sided on the border); the normal (-zx, -zy, 1)
 *   normalised; position (r / 121, c / 121, gel); lights (-0.5, 0.5, 1), (1.3, -0.4, 1), (1.3, 1.4, 1), one per channel;
 *   clip(2 n . l, 0, 1) * 255.
 * - points is depth_to_points (:154-204): with d as after the range step and xs = c - 60, ys = r - 60, the pixels with d < 1 give
 *   C . (d |xs| / 60 tan(yfov / 2) sign(xs), -d |ys| / 60 tan(yfov / 2) sign(ys), -d) + cam_pos, in row-major pixel order.
 *
 * Both launches run on `stream`; no allocation, no host synchronisation, no environment variable, no atomics, every sum in a fixed
 * order: the same bits on every call, and a view's outputs do not depend on what else is in the batch.
 *
 * What the host cannot check is made safe in the kernel, given V and F:
 * - image_mesh[i] is clamped into [0, M).
 * - face_offset entries are clamped into [0, F], and an end below its start counts as the start (an empty mesh).
 * - A face with an index outside [0, V) is skipped.
 *
 * Limits.
 * - 1 <= I <= 65536, 1 <= M <= 1048576, 0 <= V, F <= 268435456; verts may be NULL when V == 0, faces when F == 0.
 * - max_depth > 0; 0 < znear < zfar; 0 < yfov < pi.
 * - Pointers are 4-byte aligned.
 * - Anything else, or a missing required pointer, returns non-zero with a message in a3vt_last_error that names the argument and
 *   its value.  Nothing is launched. */
int a3vt_touch_render(const float *verts, int V, const int32_t *faces, int F, const int32_t *face_offset, int M, const int32_t *image_mesh,
                      const float *cam_pos, const float *cam_rot, int I, float max_depth, float yfov, float znear, float zfar, float *depth,
                      float *touch, float *points, int32_t *count, int32_t *status, void *stream);
int a3vt_touch_finish(const float *depth, const float *cam_pos, const float *cam_rot, int I, float max_depth, float yfov, float *touch,
                      float *points, int32_t *count, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The outputs of a3vt_touch_render / a3vt_touch_finish for I views in the form a data set stores them (the reference's
 * save_simulation, utility/data_making.py:186-199): images as uint8, contact clouds without their padding.
 *   touch    [I][121][121][3] fp32, or NULL       with touch_u8 [I][121][121][3] uint8 out: both or neither
 *   points   [I][14641][3] fp32, count [I] int32, status [I] int32, or all three NULL
 *            with offsets [I + 1] int32 out and cloud [capacity][3] fp32 out: all five or none
 *
 * - touch_u8 is each value clamped to [0, 255], then truncated toward zero; NaN gives 0 (so does -0).  For the values
 *   a3vt_touch_finish writes (0 <= v <= 255) that is C's (uint8_t) v, tensor.to(torch.uint8) and NumPy's .astype(np.uint8).
 * - n_i = count[i] where status[i] == 1, else 0; a count outside 0..14641 is clamped into it.  offsets is the exclusive prefix sum
 *   of n: offsets[0] = 0, offsets[I] the total.  I * 14641 <= 65536 * 14641 < 2^31.
 * - Rows [offsets[i], offsets[i + 1]) of cloud are points[i][0 .. n_i) in order, as 32-bit patterns unchanged.  Rows from
 *   offsets[I] on are not written (a3vt_touch_render's own convention for points).
 * - If offsets[I] > capacity, offsets is written in full and NO row of cloud is written: the caller reads offsets[I] and knows.
 *
 * One launch on `stream`.  No allocation, no host synchronisation, no atomics, no fence between workgroups, no workspace, no
 * environment variable: every workgroup that copies forms its prefix from count and status itself, in integers, so the result does
 * not depend on the launch geometry and is the same bits on every call.  No input is written; outputs must not overlap inputs.
 *
 * Limits.
 * - 1 <= I <= 65536; 0 <= capacity.
 * - touch is 16-byte aligned, every other pointer 4-byte aligned.  cloud may be NULL when capacity == 0.
 * - Both groups NULL, a group given in part, or anything else outside the limits returns non-zero with a message in
 *   a3vt_last_error that names touch_pack, the argument and its value.  Nothing is launched.
 *
 * a3vt_touch_pack_launches: [0] the a3vt_touch_pack calls that launched since the last reset; returns 1. */
int a3vt_touch_pack(const float *touch, const float *points, const int32_t *count, const int32_t *status, int I, int capacity,
                    uint8_t *touch_u8, int32_t *offsets, float *cloud, void *stream);
int a3vt_touch_pack_launches(long long *counts /*[1]*/, int reset);

/* ---------------------------------------------------------------------------------------------
 * The finger closing of the kinematic grasp (pterotactyl/simulator/physics/grasping.py, csrc/grasp_close.hip): from G placed hands
 * and a table of M meshes to the angles at which each finger stops, the links' poses and the finger frames.
 *
 * THE CLOSING RULE IS A KINEMATIC STAND-IN for the reference's five stepSimulation calls under position control
 * (simulator/physics/grasping.py:54-63).  It is not pybullet: no frame of it has been compared with one of pybullet's.
 *
 * The hand.  hand_table is a HOST table of 28 rows of 26 doubles, the hand's links without the base in depth-first order: four
 * chains of 7 links (rows 7 c .. 7 c + 6), the first four of a chain revolute, the last three fixed.  Columns:
 *   [0] parent row (-1: the base; otherwise a lower row of the same chain)   [1] 1 revolute, 0 fixed
 *   [2..4] the joint's origin in the parent's frame   [5..13] its rotation, row-major   [14..16] the joint's axis (unit length)
 *   [17] lower and [18] upper limit   [19] 1 when the link carries a collision box   [20..22] the box's centre and [23..25] its
 *   half-extents in the link's frame.
 * q0: a HOST table of 28 doubles, the rest angles (the entry of a fixed joint is ignored).
 * A link's pose is  R = R_parent * R_origin * Rot(axis, angle),  p = p_parent + R_parent * xyz;  the base's is base_pos[g] (3) and
 * base_rot[g] (3 x 3 row-major), DEVICE arrays.  The kernel works in float32.
 *
 * The meshes: verts (V, 3) and faces (F, 3, global vertex indices) on the DEVICE, a3vt_touch_render's layout; face_offset (M + 1)
 * and grasp_mesh (G) are HOST tables: grasp g closes on the faces [face_offset[m], face_offset[m + 1]), m = grasp_mesh[g].  A
 * face with an index outside [0, V) or a non-finite coordinate is skipped.
 *
 * The rule, for every grasp and each chain on its own (fingers do not see each other; the base is not tested).  Joint j of the
 * chain (j = 0..3, proximal to distal) has delta_j = (upper_j - q0_j) / steps and stands after k accepted steps at
 * q0_j + k * delta_j, at upper_j exactly for k = steps.  For step = 1..steps, and within a step for j = 0..3: unless joint j is
 * frozen it tries the angle of `step` steps.  The try is accepted iff no collision box of link j or of a link behind it in the
 * chain overlaps a triangle of the grasp's mesh under the tentative angles; otherwise the joint is frozen for good and
 * blocked_step[j] = step - 1, the steps it took.  A joint never blocked ends at upper_j with blocked_step[j] = steps.
 * Overlap is the 13-axis separating-axis test of an oriented box against a triangle — the box's three axes, the triangle's
 * normal, the nine cross products — in the box's frame; touching counts as overlap; a cross-product axis (the normal included)
 * whose squared length is below 1e-24 is skipped.
 *
 * Outputs (DEVICE), written for every grasp: q_out (G, 16) and blocked_step (G, 16), entry 4 c + j for joint j of chain c;
 * link_pos (G, 28, 3) and link_rot (G, 28, 3, 3), the poses of all links at q_out; frame_pos (G, 4, 3) and frame_rot (G, 4, 3, 3),
 * those of each chain's last link (the finger's camera link).  No atomics: two calls write the same bytes, and a grasp's rows do
 * not depend on the other grasps of the call.
 *
 * One launch per 64 grasps on `stream`, no host synchronisation.  G == 0 launches nothing and returns 0.
 *
 * Limits: 0 <= G <= 2^20; 1 <= M <= 2^20; 0 <= V, F <= 2^28; 1 <= steps <= 65536; face_offset starts at >= 0, does not decrease and
 * ends at <= F; grasp_mesh[g] in [0, M); the table as described above, its numbers finite, lower <= upper, half-extents >= 0.
 * Pointers 4-byte aligned (hand_table and q0: 8).  Anything else returns non-zero with a message in a3vt_last_error that names
 * grasp_close, the argument and its value.  Nothing is launched.
 *
 * a3vt_grasp_limit(which): [0] the candidate triangles a workgroup holds in LDS (more are read from global memory in every
 * query), [1] the grasps of one launch, [2] the columns of hand_table; 0 otherwise.
 * a3vt_grasp_reach: the radius of chain c's reach sphere about the chain's first joint, as the kernel's cull uses it (without
 * the 1e-4 slack), from a hand_table; negative with the message set for a table that a3vt_grasp_close would refuse.
 * a3vt_grasp_launches: [0] the a3vt_grasp_close calls that launched since the last reset (G > 0), [1] the kernels they launched;
 * returns 2. */
int a3vt_grasp_close(const float *verts, int V, const int32_t *faces, int F, const int32_t *face_offset, int M, const int32_t *grasp_mesh,
                     const float *base_pos, const float *base_rot, int G, const double *hand_table, const double *q0, int steps,
                     float *q_out, int32_t *blocked_step, float *link_pos, float *link_rot, float *frame_pos, float *frame_rot,
                     void *stream);
int a3vt_grasp_limit(int which);
double a3vt_grasp_reach(const double *hand_table, int chain);
int a3vt_grasp_launches(long long *counts /*[2]*/, int reset);

/* ---------------------------------------------------------------------------------------------
 * The hand's placement on the convex hull of a mesh's vertices, without a hull (pterotactyl/simulator/physics/grasping.py::place_hand,
 * csrc/hull_place.hip): the base pose of the hand for each of A actions on each of M meshes.
 *
 * place_hand uses only the farthest point t d of the ray from the origin along the action's direction d that is still inside the
 * convex hull, and the plane of the facet there.  That is a linear programme in three variables: the largest t with t d in the
 * convex hull of the vertices.  Its optimal basis is three vertices that span the facet.  It is solved by SUPPORT PASSES — the
 * lowest index i of the largest n . v_i over the mesh's vertices — and no hull is built.
 *
 * The meshes: verts (V, 3) fp32 on the DEVICE; vert_offset (M + 1) a HOST table: mesh m owns the vertices vert_offset[m] ..
 * vert_offset[m + 1] - 1, ALL of them, referenced by a face or not (as place_hand takes them).  directions (A, 3) and tip_offset
 * (3) are HOST tables of doubles; d = directions[a] is used as given, not normalised, and t is in units of it.
 *
 * The rule, per mesh m and action a.  All arithmetic is float64 on the fp32 vertices converted exactly; no multiply-add is fused;
 * a dot product is (n.x v.x + n.y v.y) + n.z v.z.
 * 0. A mesh with fewer than 4 vertices or a non-finite coordinate: status 1 (place_hand returns None).  This check comes first.
 * 1. Frame.  e = the coordinate axis of d's smallest |component| (the lowest axis on a tie); x = (d x e) / |d x e|,
 *    y = (d x x) / |d x x|.  The projection of vertex v_i is p_i = (v_i . x, v_i . y).  The support along a 2-D direction u is the
 *    support pass of n = u.x x + u.y y, and its support value is p_w . u of the winning vertex w.
 * 2. Phase 1, a 2-D GJK on the p_i: a = support along (1, 0): p_a.x < 0 is status 1, p_a.x == 0 status 2.  b = support along
 *    -p_a.  Then, up to 32 times: c = support along the normal of edge a b that faces the origin, (-e.y, e.x) or its negative for
 *    e = p_b - p_a, by the sign of e.y p_a.x - e.x p_a.y.  With o_ac = (p_c - p_a) x (-p_a), b_ac = (p_c - p_a) x (p_b - p_a) and
 *    o_bc, a_bc alike for edge b c: if o_ac and b_ac differ in sign the origin is outside edge a c, and c replaces b; else if o_bc
 *    and a_bc differ, c replaces a; else the triangle's projection holds the origin and phase 1 ends.
 *    Every support value below 0 is a separating direction: status 1, the ray misses.  Exact ties are status 2: a support value of
 *    0, a support vertex already in the simplex, the origin on the line of the edge, one of the four cross products 0, the pass cap.
 *    One exception: on the OPENING edge (a, b straight from the two opening supports) the origin on the edge's line is no tie — it
 *    lies strictly between a and b since p_b . (-p_a) > 0 — and the search goes on along (-e.y, e.x).  That is the case of every
 *    mesh that is symmetric about the origin, where b is a's antipode.
 * 3. Phase 2, pivots, up to 64 times: N = (b - a) x (c - a), n = N / (N . d) (N . d == 0: status 2), t = n . a.  w = the support
 *    pass of n, hi / lo the largest / smallest n . v_i.  If hi <= t or w is in the basis, the basis is optimal.  Otherwise w enters
 *    and one vertex leaves by the ratio test: with area = (p_b - p_a) x (p_c - p_a) (0: status 2), lambda = (p_b x p_c, p_c x p_a,
 *    p_a x p_b) / area clamped from below at 0 and mu = ((p_b - p_w) x (p_c - p_w), (p_c - p_w) x (p_a - p_w), (p_a - p_w) x
 *    (p_b - p_w)) / area, the vertex k with the smallest lambda_k / mu_k over mu_k > 0 leaves (the first on a tie; none: status 2).
 *    The pass cap is status 2.
 * 4. Checks, in order: t <= 0 is status 1 (the line meets the hull behind the origin); hi - lo <= 1e-12 x the mesh's largest
 *    |coordinate| is status 2 (a flat hull, which Qhull refuses; hi and lo are the last pass's, so this costs no pass).
 * 5. The pose, place_hand line for line: point = d t; normal = N / |N|, negated if |point|^2 > |point + 1e-4 normal|^2;
 *    position = point + hand_distance normal; normal -= 0.001 per component; b = normal / |normal|; with v = (-1, 0, 0) x b,
 *    c = -b.x, s^2 = b.z^2 + b.y^2 and K the cross-product matrix of v: R = I + K + K K ((1 - c) / s^2); s^2 < 1e-24 is status 2
 *    (the reference's reflection case); base_pos = position - R tip_offset.  (place_hand's quaternion round trips change R by
 *    about 1e-16 and are not restated.)
 *
 * Outputs (DEVICE), written for every pair, row m A + a: status int32 — 0 placed, 1 no intersection (place_hand's None), 2 not
 * decided here: the caller asks place_hand; base_pos (3) and base_rot (3 x 3, row-major) fp32, the float64 pose rounded once;
 * simplex (3) int32, the basis's vertices as indices WITHIN the mesh; t float64.  Rows with status != 0 are zeros, simplex -1.
 * No atomics: two calls write the same bytes, and a pair's row does not depend on the rest of the batch.
 *
 * One workgroup per pair, one launch per 128 meshes (all pairs in ONE launch for M <= 128: the directions and the launch's
 * vertex ranges travel in the kernel arguments) on `stream`, no host synchronisation.
 *
 * Limits: 1 <= M <= 2^20; 1 <= A <= 128; M A <= 2^20; 0 <= V <= 2^28; vert_offset starts at >= 0, does not decrease and ends at
 * <= V; directions, tip_offset and hand_distance finite, no direction zero.  Pointers non-NULL (verts may be NULL when V == 0)
 * and 4-byte aligned (directions, tip_offset and t: 8).  Anything else returns non-zero with a message in a3vt_last_error that
 * names hull_place, the argument and its value.  Nothing is launched.
 *
 * a3vt_hull_place_launches: [0] the a3vt_hull_place calls that launched since the last reset, [1] the kernels they launched;
 * returns 2. */
int a3vt_hull_place(const float *verts, int V, const int32_t *vert_offset, int M, const double *directions, int A, double hand_distance,
                    const double *tip_offset, int32_t *status, float *base_pos, float *base_rot, int32_t *simplex, double *t, void *stream);
int a3vt_hull_place_launches(long long *counts /*[2]*/, int reset);

/* ---------------------------------------------------------------------------------------------
 * The ground-truth point cloud of a mesh: utility/data_making.py::extract_points (mesh_to_voxel, extract_ODMs, apply_ODMs,
 * voxel_to_pointcloud, realign_points of utility/utils.py) for a batch of M meshes.
 *
 *   verts        [V][3] fp32, the meshes' vertices concatenated
 *   faces        [F][3] int32, the meshes' faces concatenated, each with indices LOCAL to its mesh (as the mesh's file stores them)
 *   vert_offset  [M + 1] int32: mesh m owns vertices vert_offset[m] .. vert_offset[m + 1] - 1
 *   face_offset  [M + 1] int32: the same for faces
 *   dim          the grid's resolution; a grid is [dim][dim][dim] bytes, (i, j, k) = (x, y, z), k fastest
 *
 * a3vt_voxel_surface: everything up to the size of each mesh's surface.
 * - Normalisation.  n(v) = (v - lo) / (hi - lo) - 0.5 in fp32, each step rounded, lo / hi the smallest / largest FINITE coordinate
 *   of the mesh's vertices, used or not, over all three axes.
 * - Subdivision.  A triangle (a, b, c) is split while its largest squared side exceeds (float)((1.0 / dim)^2): strictly, the squared
 *   side being ((dx dx + dy dy) + dz dz) with every step rounded.  Its children are (a, ac, ab), (ab, b, bc), (ab, ac, bc),
 *   (ac, c, bc) with ab = (a + b) / 2 and so on.  The test is per triangle, so siblings stop at different depths.  A triangle of
 *   depth 12 is never split (no finite input reaches it: the depth is at most ceil(log2(sqrt(3) dim)) + 1 <= 10).
 * - Marking.  Every face's three vertices and every midpoint formed mark voxel trunc((p + 0.5) * (dim - 1)) per axis, fp32, each step
 *   rounded.  A face with an index outside its mesh, or with a non-finite normalised coordinate, marks nothing.
 * - occupancy [M][dim][dim][dim] uint8 out, or NULL: the marked grid (mesh_to_voxel's).
 * - depth_maps [M][6][dim][dim] int32 out, or NULL: extract_ODMs' values — see a3vt_voxel_depth_maps.
 * - Carving.  A voxel is kept iff along each of the three axes it lies inside [first, last] occupied voxel of its column.  This equals
 *   apply_ODMs INCLUDING its binary_fill_holes: a carved voxel lies outside its column's interval along some axis, and so does
 *   every voxel beyond it in that column out to the border, so no carved region is enclosed.
 * - Surface.  A kept voxel with fewer than 27 kept voxels in its 3 x 3 x 3 neighbourhood, voxels outside the grid counting as empty
 *   (voxel_to_pointcloud).  counts [M] int32 out: the number of surface voxels of each mesh.
 * The tables the next call needs (kept grids, row offsets, the surface's and the vertices' per-axis bounds) stay in the library's
 * workspace: one per device, grown with hipMalloc when a call needs more than any before it (the only allocation; it may
 * synchronise the device), and cleared by every call — nothing of an earlier call's grids is visible to a later one.  Calls that share
 * a device must therefore be made in order, from one thread at a time, on one stream.
 *
 * a3vt_voxel_points: the clouds, from the workspace of the a3vt_voxel_surface call right before it (same M and dim, else an error).
 * - total: the sum of that call's counts, which the caller read from the device (the one host read the pipeline needs: the size of
 *   `surface` depends on it).
 * - surface [total][3] int32 out: the surface voxels (i, j, k), mesh after mesh, each mesh's in lexicographic order (torch.where's).
 * - aligned [total][3] fp32 out, or NULL: realign_points of every row.  Per axis, in fp32 with every step rounded, lo / hi the
 *   surface's smallest / largest index on that axis of that mesh: mid = (hi + lo) / 2; c = x - mid; range = ((hi - mid) + 1) - (lo - mid);
 *   result = (c * (vhi - vlo)) / range, vlo / vhi the smallest / largest finite vertex coordinate of the mesh on that axis.
 * - cloud [M][num_points][3] fp32 out with index [M][num_points] int64, both or neither: row p of mesh m is the realigned surface
 *   row index[m][p] mod n_m of that mesh — "mod" because the reference doubles a cloud of n_m rows until it has num_points, and row r
 *   of a doubled cloud is row r mod n_m.  A mesh with n_m = 0 gets zeros.
 *
 * a3vt_voxel_depth_maps: extract_ODMs on grids the caller supplies.  voxels [M][dim][dim][dim] uint8, non-zero = occupied.
 * depth_maps [m][0][i][j] = dim - 1 - (last occupied k of column (i, j)), [1][i][j] = its first occupied k; [2], [3] the same along j
 * for column (i, k); [4], [5] along i for column (j, k); dim for an empty column.
 *
 * Launches per call do not depend on M, the number of faces or the subdivision depth: a3vt_voxel_surface enqueues the clear and seven
 * kernels (six without faces; one copy more for each optional output), a3vt_voxel_points two kernels, a3vt_voxel_depth_maps one.
 * Nothing synchronises the host.  Marking is a plain store of 1, the surface's bounds are integer atomics, every float step is
 * rounded on its own (the file is compiled without contraction): the same bits on every call, whatever else is in the batch.
 * a3vt_voxel_launches: operations enqueued since the last reset by [0] a3vt_voxel_surface, [1] a3vt_voxel_depth_maps,
 * [2] a3vt_voxel_points; returns 3.
 *
 * What the host cannot check is made safe in the kernel: offsets are clamped into [0, V] / [0, F], and an end below its start
 * counts as the start (an empty mesh); writes to `surface` stop at `total`.
 *
 * Limits.
 * - 4 <= dim <= 256, 1 <= M <= 4096, M * dim^3 <= 2^30, 0 <= V, F <= 268435456, 0 <= total <= 2^30, 1 <= num_points <= 268435456.
 * - verts may be NULL when V == 0, faces when F == 0, surface when total == 0.
 * - Pointers are 4-byte aligned, index 8-byte aligned; the byte grids need no alignment.
 * - Anything else, or a missing required pointer, returns non-zero with a message in a3vt_last_error that names the argument and
 *   its value.  Nothing is launched. */
int a3vt_voxel_surface(const float *verts, int V, const int32_t *faces, int F, const int32_t *vert_offset, const int32_t *face_offset, int M,
                       int dim, uint8_t *occupancy, int32_t *depth_maps, int32_t *counts, void *stream);
int a3vt_voxel_depth_maps(const uint8_t *voxels, int M, int dim, int32_t *depth_maps, void *stream);
int a3vt_voxel_points(int M, int dim, long long total, int32_t *surface, float *aligned, const long long *index, int num_points, float *cloud,
                      void *stream);
int a3vt_voxel_launches(long long *counts /*[3]*/, int reset);

/* ---------------------------------------------------------------------------------------------
 * Mesh and point-cloud rendering: what utility/pretty_render.py asks of pyrender, as a ray caster of this library's own.
 *
 * THIS IS NOT PYRENDER'S SHADER.  It is ray casting at pixel centres with Lambert shading under the reference's lights and camera.
 * It is not the metallic-roughness model, and no image of it has been compared with one of pyrender's.
 *
 * One call renders I images.  Every image has its own pinhole camera and looks at one of M scenes cut from shared tables.
 *   verts         [V][3] fp32 and faces [F][3] int32 (indices into verts, already global), face_rgb [F][3] uint8: the triangles
 *   centres       [S][3] fp32, radii [S] fp32, sphere_rgb [S][3] uint8: the spheres
 *   face_offset   [M + 1] int32, HOST: scene m owns faces face_offset[m] .. face_offset[m + 1] - 1
 *   sphere_offset [M + 1] int32, HOST: the same for spheres.  A scene may be empty.
 *   image_scene   [I] int32, HOST: the scene image i looks at
 *   cam_pos       [I][3], cam_rot [I][3][3] fp32: the camera's pose matrix as pretty_render.py builds it.  The camera looks down its
 *                 own -z; no R_y(-90 deg) is applied (unlike a3vt_touch_render's finger frame).
 *   yfov (radians), znear, zfar, W, H: the aspect ratio is W / H
 *   lights        [L][4] fp32, HOST: position (world) and intensity; ambient; background [3] uint8, HOST
 *   rgb           [I][H][W][3] uint8 out
 *   depth         [I][H][W] fp32 out: 0 without a hit
 *   prim          [I][H][W] int32 out, or NULL: the face's index, F + the sphere's index, -1 without a hit (indices into the tables)
 * The HOST tables are small; they are read and checked during the call and travel in the kernel arguments, which is what lets the
 * call refuse a bad table before anything is launched and without reading the device.  Everything else is device memory.
 *
 * Visibility.
 * - Pixel (r, c), row 0 at the top, has the centre x = (c + 0.5) / W * 2 - 1, y = 1 - (r + 0.5) / H * 2 and the ray
 *   (x tan(yfov / 2) W / H, y tan(yfov / 2), -1) in the eye frame, as in the touch contract.
 * - depth is the ray parameter (= -z in the eye frame) of the nearest hit with znear <= depth <= zfar.
 * - Triangles are two-sided and inclusive on edges.  Across an edge that two faces share BY VERTEX INDEX the test is watertight
 *   (a3vt_touch_render's rule, restated in csrc/scene_render.hip).
 * - A sphere of centre c and radius r is hit, with oc = c - o and the unit ray u, at b - sqrt(disc), b = oc . u,
 *   disc = r^2 - |oc - b u|^2 >= 0; a ray that starts inside a sphere does not hit it (its only hit lies behind it or is the far one).
 * - Among hits of exactly equal depth the lowest prim wins, so the output does not depend on chunking or order of evaluation.
 *   A face's depth is computed from its vertices in the order of their indices: copies of a face under another winding or
 *   rotation (add_faces' (a, c, b) and (c, b, a)) have exactly the depth of the original, and the first of them is seen.
 * - A face with a non-finite coordinate, a sphere with a non-finite centre or radius or with radius <= 0, is never hit and changes
 *   nothing else.  A face with an index outside [0, V) is skipped: this is checked on the device, as a3vt_touch_render does.
 *
 * Shading, in fp32, of the hit point p.
 * - n is the unit face normal turned towards the eye, or (p - c) / r on a sphere.
 * - out = clip(base * (ambient + (1 / pi) sum_k I_k max(0, n . l_k / |l_k|) / |l_k|^2), 0, 255) per channel, l_k = L_k - p, the sum
 *   in table order, rounded half up.  No shadows, no specular term, no vertex normals, no blending.  A pixel without a hit gets
 *   the background.
 *
 * One launch per 128 images (a reference-sized job, 16 objects of 3 images, is one), on `stream`; a workgroup takes a 16 x 16 tile.
 * No allocation, no host synchronisation, no atomics, every float sum in a fixed order: the same bits on every call, and an
 * image does not depend on what else is in the batch.
 * a3vt_scene_launches: since the last reset, [0] the a3vt_scene_render calls that were accepted, [1] the kernels they launched;
 * returns 2.
 *
 * Limits.
 * - 1 <= I <= 65536, 1 <= M <= 1048576, 1 <= W, H <= 2048, 0 <= L <= 8, 0 <= V, F, S <= 268435456.
 * - verts and centres / radii may be NULL when V == 0 or S == 0, faces and face_rgb when F == 0, sphere_rgb when S == 0, lights when
 *   L == 0.
 * - 0 < znear < zfar < infinity; 0 < yfov < pi; ambient finite.
 * - face_offset and sphere_offset start at >= 0, do not decrease and end at <= F and <= S; image_scene[i] lies in [0, M).
 * - Pointers to fp32 and int32 are 4-byte aligned; the byte tables need no alignment.
 * - Anything else, or a missing required pointer, returns non-zero with a message in a3vt_last_error that names the argument and
 *   its value.  Nothing is launched. */
int a3vt_scene_render(const float *verts, int V, const int32_t *faces, const uint8_t *face_rgb, int F, const float *centres,
                      const float *radii, const uint8_t *sphere_rgb, int S, const int32_t *face_offset, const int32_t *sphere_offset,
                      int M, const int32_t *image_scene, const float *cam_pos, const float *cam_rot, int I, float yfov, float znear,
                      float zfar, int W, int H, const float *lights, int L, float ambient, const uint8_t *background, uint8_t *rgb,
                      float *depth, int32_t *prim, void *stream);
int a3vt_scene_launches(long long *counts /*[2]*/, int reset);

/* ---------------------------------------------------------------------------------------------
 * Scenes of posed instances: the vision scene with the hand in it (simulator/rendering/vision_renderer.py's update_hand + render;
 * Sampler.sample's vision_occluded), without writing the posed triangles out.
 *
 * THIS IS NOT PYRENDER'S SHADER: it is a3vt_scene_render's ray caster.  The digit's alpha is not blended.  No image of it has been
 * compared with one of pyrender's.
 *
 * An INSTANCE is a part, a rigid pose and a colour.  A part is a face range of a shared template table.  An image's object is an
 * instance under the identity pose, the Allegro hand 21 more.
 *   part_verts       [PV][3] fp32 and part_faces [PF][3] int32 (indices into part_verts, already global): the templates
 *   part_face_offset [P + 1] int32, HOST: part p owns the faces part_face_offset[p] .. part_face_offset[p + 1] - 1
 *   part_bound       [P][4] fp32, HOST: centre and radius of a sphere that holds every finite vertex the part's faces use
 *   inst_part        [N] int32, inst_pos [N][3], inst_rot [N][3][3] fp32 (row-major), inst_rgb [N][3] uint8: the instances
 *   inst_offset      [I + 1] int32, HOST: image i owns the instances inst_offset[i] .. inst_offset[i + 1] - 1; the range may be empty
 *   cam_pos, cam_rot, yfov, znear, zfar, W, H, lights, L, ambient, background, rgb, depth: exactly a3vt_scene_render's
 *   prim_inst        [I][H][W] int32 out, or NULL: the global instance index (into inst_part), -1 without a hit
 *   prim_face        [I][H][W] int32 out, or NULL: the face's index into part_faces, -1 without a hit.  Both or neither.
 *
 * The rule.
 * - A template vertex v of an instance with the pose (R, p) becomes, per row r,
 *     w_r = fmaf(R[r][0], v.x, fmaf(R[r][1], v.y, fmaf(R[r][2], v.z, p[r]))).
 *   R is used as given: nothing checks that it is a rotation, so a scale or a shear poses the part as the formula says.
 * - From w on everything is a3vt_scene_render's rule, word for word and by the same device code (csrc/scene_dev.h): the camera
 *   transform, the rounded edge functions oriented by vertex index, the plane from the vertices in index order, two-sided, inclusive
 *   edges, the depth range, Lambert shading of the winner read again by its indices, with the instance's colour.
 * - Among hits of exactly equal depth the lower (instance index, face index) wins.
 * - An instance is skipped as a whole if its part id lies outside [0, P) or an entry of its pose is not finite: this is checked on
 *   the device.  A face with a non-finite posed coordinate, or with an index outside [0, PV), is skipped and changes nothing else.
 * Consequence: rgb and depth equal, bit for bit, what a3vt_scene_render gives for the triangles a3vt_pose_parts writes out, and
 * (prim_inst, prim_face) is that call's prim under the materialised numbering.
 *
 * Culling is conservative for ANY finite R: an instance is bounded by its part's sphere with the centre posed like a vertex and the
 * radius scaled by the Frobenius norm of R (>= the largest stretch of R), faces then one by one as in a3vt_scene_render.
 *
 * One launch per 128 images on `stream`; a workgroup takes a 16 x 16 tile.  No allocation, no workspace, no host synchronisation, no
 * atomics: the same bits on every call, and an image does not depend on what else is in the batch.
 *
 * a3vt_pose_parts: the materialised formulation, one launch.  Instance n writes, with the same device function, its part's posed
 * vertices to verts_out[vert_base[n] ..], its part's faces re-based onto them to faces_out[face_base[n] ..] and its colour once per
 * face to face_rgb_out.  part_vert_offset [P + 1] int32, HOST: part p owns the vertices part_vert_offset[p] .. part_vert_offset[p + 1]
 * - 1 of part_verts; a face index outside its own part's vertices is written as -1 (a3vt_scene_render skips such a face).  vert_base
 * and face_base are [N + 1] int32 on the DEVICE, the caller's running sums; an instance whose part id is out of range, or whose
 * ranges do not have its part's sizes or leave [0, TV) / [0, TF), writes nothing.
 * a3vt_posed_launches: since the last reset, [0] the a3vt_scene_render_posed calls that were accepted, [1] the kernels they launched,
 * [2] the kernels of a3vt_pose_parts; returns 3.
 *
 * Limits.
 * - 1 <= I <= 65536, 1 <= P <= 96, 0 <= N <= 16777216, 1 <= W, H <= 2048, 0 <= L <= 8, 0 <= PV, PF, TV, TF <= 268435456.
 * - The instance tables may be NULL when N == 0, part_verts / part_faces when PV == 0 / PF == 0, lights when L == 0.
 * - 0 < znear < zfar < infinity; 0 < yfov < pi; ambient finite; part_bound finite with a radius >= 0.
 * - part_face_offset, part_vert_offset and inst_offset start at >= 0, do not decrease and end at <= PF, <= PV and <= N.
 * - Pointers to fp32 and int32 are 4-byte aligned; the byte tables need no alignment.
 * - Anything else, or a missing required pointer, returns non-zero with a message in a3vt_last_error that names the argument and
 *   its value.  Nothing is launched. */
int a3vt_scene_render_posed(const float *part_verts, int PV, const int32_t *part_faces, int PF, const int32_t *part_face_offset,
                            const float *part_bound, int P, const int32_t *inst_part, const float *inst_pos, const float *inst_rot,
                            const uint8_t *inst_rgb, int N, const int32_t *inst_offset, const float *cam_pos, const float *cam_rot, int I,
                            float yfov, float znear, float zfar, int W, int H, const float *lights, int L, float ambient,
                            const uint8_t *background, uint8_t *rgb, float *depth, int32_t *prim_inst, int32_t *prim_face, void *stream);
int a3vt_pose_parts(const float *part_verts, int PV, const int32_t *part_faces, int PF, const int32_t *part_vert_offset,
                    const int32_t *part_face_offset, int P, const int32_t *inst_part, const float *inst_pos, const float *inst_rot,
                    const uint8_t *inst_rgb, int N, const int32_t *vert_base, const int32_t *face_base, float *verts_out, int TV,
                    int32_t *faces_out, uint8_t *face_rgb_out, int TF, void *stream);
int a3vt_posed_launches(long long *counts /*[3]*/, int reset);

/* ---------------------------------------------------------------------------------------------
 * The supervised latent policy's value network (policies/supervised/model.py, train.py:119-158), fp32 throughout.
 *
 * The network is a table of at most 16 layers, read on the host and passed to the kernels by value.  Layer l computes
 * y[o] = act(sum_i weight[o][i] x[i] + bias[o]) with weight [out][in] row-major (torch's Linear layout, used in place) and act = ReLU
 * when relu != 0.  The input of layer 0 is mask[e] (layer[0].in columns).  The input of layer concat_at (1 <= concat_at < n_layers) is
 * cat(output of the layer before, latent[e], first_latent[e]), latent and first_latent [rows][latent_size]; every other layer reads
 * the layer before it, so in must equal that layer's out (at concat_at: out + 2 * latent_size).  transform 0 leaves the last layer's
 * output z as it is (DDQN's Latent_Model); transform 1 gives sigmoid(z) * scale - offset, sigmoid(z) = 1 / (1 + expf(-z)), the product
 * and the difference rounded separately.
 *
 * Arithmetic contract of the forward.  Each output neuron is ONE fixed-order sum: lane l of a 64-lane wave owns the columns
 * W (64 i + l) .. W (64 i + l) + W - 1, i = 0, 1, .., with W = 4 (16-byte loads) when in % 4 == 0 and W = 1 otherwise; it adds its
 * products to a zero accumulator in ascending column order, one fused multiply-add per term; the 64 partial sums are added by the
 * butterfly v += shfl_xor(v, 32), 16, 8, 4, 2, 1; the bias is added last; then the ReLU (x < 0 ? 0 : x, a NaN stays).  A row's result
 * therefore depends neither on rows nor on the row's position: the same bits for a row evaluated alone, with rows appended, or
 * permuted.  Activations stay in LDS between layers; a row is one workgroup.
 *
 * a3vt_latent_policy_fwd: one launch.  values [rows][A], A = the last layer's out, always written, unmasked.  With `taken`
 * ([rows][A] fp32) `action` [rows] int32 is required and receives the action choice: the index of the lowest value among the actions
 * with taken[e][a] == 0; a tie (-0 == +0 included) goes to the lower index, a NaN sorts after +inf, -1 when no action is open — the
 * ordering rule of a3vt_latent_nearest.  With `stash` ([rows][a3vt_latent_policy_stash_floats(net)]) every layer's post-activation
 * row is kept for the backward, layer after layer; for transform 1 the last layer's entry is sigmoid(z).
 *
 * a3vt_action_value_loss: one launch.  values [rows][A], actions [steps][rows] int32, targets [steps][rows] ->
 * loss[0] = (1 / (steps rows)) sum_{t,e} (targets[t][e] - values[e][actions[t][e]])^2, summed in a fixed order, and dvalues [rows][A]
 * = its gradient: zero, then for t ascending dvalues[e][a] += (values[e][a] - targets[t][e]) * (2 / (steps rows)), so repeated (e, a)
 * pairs add up in t order.  The caller guarantees 0 <= actions < A (the Python layer refuses others); the kernel skips such a pair
 * rather than index outside the row.
 *
 * a3vt_latent_policy_bwd: two launches.  (1) per row: delta of the last layer = dvalues * scale * s (1 - s) for transform 1 (s from
 * the stash), dvalues otherwise; then delta_{l-1}[i] = relu'(stash_{l-1}[i] > 0) * sum_o weight_l[o][i] delta_l[o], one thread per
 * column i, o ascending, one fused multiply-add per term; at concat_at only the columns of the previous layer flow on.  All deltas go
 * to `delta` (the stash's shape).  (2) over (layer, slab of 8 output rows): dweight[o][i] = sum_e delta[e][o] x[e][i] (fused
 * multiply-adds) and dbias[o] = sum_e delta[e][o], e ascending; accumulate != 0 adds the sums to what the gradient tensors hold,
 * accumulate == 0 overwrites.  There are no gradients for mask, latent or first_latent.
 *
 * Limits (a3vt_latent_policy_limit: 0 rows and steps 4096, 1 every in / out — so also out + 2 * latent_size — 1024, 2 layers 16).
 * Anything else, layers that do not chain, a null or misaligned pointer (weights 16 bytes where in % 4 == 0, everything else 4)
 * returns non-zero with a message that names the value, and launches nothing.  No atomics, no fence between workgroups, no host
 * synchronisation, no allocation: the same bits on every call.  a3vt_latent_policy_launches: kernel launches of the three entry
 * points since the last reset ([0] forward, [1] loss, [2] backward); returns 3. */
typedef struct a3vt_mlp_layer {
  const float *weight, *bias;
  int32_t in, out, relu, reserved;
} a3vt_mlp_layer;
typedef struct a3vt_mlp {
  a3vt_mlp_layer layer[16];
  int32_t n_layers, concat_at, latent_size, transform;
  float scale, offset;
} a3vt_mlp;
typedef struct a3vt_mlp_grads {
  float *dweight[16], *dbias[16];
} a3vt_mlp_grads;
int a3vt_latent_policy_limit(int which);
int a3vt_latent_policy_stash_floats(const a3vt_mlp *net);   /* per row; 0 for a table the entry points refuse */
int a3vt_latent_policy_fwd(const a3vt_mlp *net, const float *mask, const float *latent, const float *first_latent, const float *taken,
                           int rows, float *values, int32_t *action, float *stash, void *stream);
int a3vt_action_value_loss(const float *values, const int32_t *actions, const float *targets, int steps, int rows, int num_actions,
                           float *loss, float *dvalues, void *stream);
int a3vt_latent_policy_bwd(const a3vt_mlp *net, const a3vt_mlp_grads *grads, const float *mask, const float *latent,
                           const float *first_latent, const float *dvalues, const float *stash, float *delta, int rows, int accumulate,
                           void *stream);
int a3vt_latent_policy_launches(long long *counts /*[3]*/, int reset);

/* DDQN's Latent_Model (policies/DDQN/model.py:15-61) on the layer table above: an a3vt_mlp with transform 0 whose last layer has
 * A <= 304 outputs (the actions).  The forward, the deltas and the gradients are the sums of a3vt_latent_policy_fwd / _bwd, the TD rule
 * is a3vt_ddqn_td's — the same device code, not a second summation order.
 *
 * a3vt_ddqn_latent_q: one launch.  q [rows][A] always written, unpenalised: bit-identical to a3vt_latent_policy_fwd's values.  With
 * mask_penalty ([rows][A] fp32; the observation's mask) `action` [rows] int32 is required and receives
 * argmax_a (mask_penalty[e][a] > 0 ? -1e10 : q[e][a]) under a3vt_ddqn_td's rule: the lowest index on a tie, so index 0 when every
 * action is taken.  mask_penalty and action are NULL together.
 *
 * a3vt_ddqn_latent_update: one update's device work as three launches.  `online` and `target_net` are two tables of the same layer
 * sizes; mask, mask_n [batch][layer[0].in] (mask is also the [batch][A] table of taken actions: layer[0].in == A for this model, and
 * the entry point reads A columns of it), latent, latent_n, first_latent [batch][latent_size]; actions [batch] fp32, clamped into
 * [0, A) as in a3vt_ddqn_td; rewards [batch]; denom [batch] or NULL.
 *   (1) a batch x 3 grid of workgroups, one role each: online(mask, latent) -> q_cur with the stash kept, online(mask_n, latent_n),
 *       target_net(mask_n, latent_n); first_latent is shared.
 *   (2) a workgroup per row: a3vt_ddqn_td's sample rule (penalised by the CURRENT mask, target = fadd(fmul(gamma, next), reward)) ->
 *       best_next, target_out, diff; dq[a] = (1 * 2 * diff) / batch at the action and 0 elsewhere, kept in LDS; then the deltas of
 *       a3vt_latent_policy_bwd (1), every term summed, zero ones too.
 *   (3) a workgroup per (layer, slab of 8 rows): dweight / dbias of a3vt_latent_policy_bwd (2), overwriting; one more workgroup
 *       reduces loss[0] = mean(diff^2) by a3vt_ddqn_td's pairwise tree.
 * Every output (q_cur [batch][A], best_next, target_out, diff [batch], loss [1], the gradients) is bit-identical to
 * a3vt_latent_policy_fwd x 3, a3vt_ddqn_td, a3vt_ddqn_td_bwd with grad_loss = 1 and a3vt_latent_policy_bwd with accumulate = 0 on the
 * same operands.  scratch: a3vt_ddqn_latent_scratch_bytes(online, batch) bytes, caller-provided (0 for a refused table or batch).
 *
 * Limits: those of a3vt_latent_policy_* for the tables (widths <= 1024, 16 layers) and of a3vt_ddqn_td (batch, rows <= 4096,
 * A <= 304).  Anything else, transform != 0, tables that differ in a layer size, a null required pointer or a misaligned one (weights 16
 * bytes where in % 4 == 0, everything else 4) returns non-zero with a message that names the value, and launches nothing.  No atomics,
 * no fence between workgroups, no host synchronisation, no allocation: the same bits on every call.
 * a3vt_ddqn_latent_launches: kernel launches since the last reset ([0] a3vt_ddqn_latent_q, [1] a3vt_ddqn_latent_update); returns 2. */
size_t a3vt_ddqn_latent_scratch_bytes(const a3vt_mlp *online, int batch);
int a3vt_ddqn_latent_q(const a3vt_mlp *net, const float *mask, const float *latent, const float *first_latent, const float *mask_penalty,
                       int rows, float *q, int32_t *action, void *stream);
int a3vt_ddqn_latent_update(const a3vt_mlp *online, const a3vt_mlp *target_net, const a3vt_mlp_grads *grads, const float *mask,
                            const float *mask_n, const float *latent, const float *latent_n, const float *first_latent,
                            const float *actions, const float *rewards, const float *denom, int batch, int budget, float gamma,
                            float *q_cur, int32_t *best_next, float *target_out, float *diff, float *loss, void *scratch, void *stream);
int a3vt_ddqn_latent_launches(long long *counts /*[2]*/, int reset);

/* Graph_Model's features and layer 0 (policies/DDQN/model.py:100-118) without the (batch * n_vert) x 300 feature rows:
 *   y = relu(layer0([a_b | PE(p) | E[token]])) = relu(agg(S[b] + T[token] + relu(L2(relu(L1(nerf(p) ++ p)))) C))
 * with the composites S = a Wa + b3 Wp [batch][npad], T = E Wm [4][npad], C = W3^T Wp [50][npad] formed by the caller
 * (npad = hidden rounded up to 4, pad columns zero; Wa / Wp / Wm = the three 100-row blocks of the layer's weight, L3 = (W3,
 * b3) the positional encoder's last Linear).  mesh [batch][n_vert][4] = x, y, z and the mask token (0..3) as a float, the
 * observation's layout; w1 [25][63], b1 [25], w2 [50][25], b2 [50] the encoder's first two Linear layers.  "agg": the first
 * cut_len columns are aggregated over the CSR and take `bias`, the rest pass through, then the ReLU — a3vt_gcn_layer_fwd with
 * relu = 1.  Exact fp32 throughout.  y [batch * n_vert][ld_y], ld_y % 4 == 0.  hidden <= 304.  mesh, the composites and the
 * scratch (a3vt_qnet_input_scratch_bytes, backward != 0 for _bwd) are 16-byte aligned.
 * a3vt_qnet_input_bwd: from grad_y and the forward's y, writes d_s [batch][npad], d_t [4][npad], d_c [50][npad], dw1, db1, dw2,
 * db2 and grad_bias [hidden]; every sum has a fixed order (same bits on every call).  There is no position gradient. */
size_t a3vt_qnet_input_scratch_bytes(int batch, int n_vert, int hidden, int cut_len, int backward);
int a3vt_qnet_input_fwd(const float *mesh, const float *w1, const float *b1, const float *w2, const float *b2, const float *comp_s,
                        const float *comp_t, const float *comp_c, const float *bias, int hidden, int cut_len, const int32_t *rowptr,
                        const int32_t *col, const float *val, int max_degree, int n_vert, int batch, float *y, int ld_y,
                        float *scratch, void *stream);
int a3vt_qnet_input_bwd(const float *mesh, const float *w1, const float *b1, const float *w2, const float *b2, const float *comp_c,
                        int hidden, int cut_len, const int32_t *rowptrT, const int32_t *colT, const float *valT, int max_degreeT,
                        int n_vert, int batch, const float *y, int ld_y, const float *grad_y, int ld_gy, float *d_s, float *d_t,
                        float *d_c, float *dw1, float *db1, float *dw2, float *db2, float *grad_bias, float *scratch, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Deferred finite check (replaces the blocking NaN trap of model.py:326-329): sets *flag (device
 * int32, caller-zeroed) to 1 if any of the n floats is NaN/Inf.  No host sync. */
int a3vt_check_finite(const float *data, size_t n, int32_t *flag, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement aid (no reference counterpart): when enabled, every fp32-MFMA launch of the GCN stack is
 * bracketed by a HIP event pair on its launch stream.  a3vt_profile_read synchronises on those events
 * and returns, per kernel class, the summed device time and launch count since the last read:
 *   [0] forward product Z = X W (hidden layers, 300x300 and the first layer)
 *   [1] backward product dX = dZ W^T (hidden layers)     [2] backward product dW = X^T dZ
 * Only hidden x hidden launches are of the headline shape; bench.py divides by the counts it expects. */
int a3vt_profile_enable(int on);
int a3vt_profile_read(double *total_ms /*[3]*/, int *count /*[3]*/);
/* The same for n classes (round 6; every call of this library on a step, so that a bench line can say where a step's time
 * goes without a profiler): [0..2] as above, [3] neighbour aggregation of the hidden layers (forward and A^T backward),
 * [4] output layer (300 -> 3 product, its aggregation, their backward), [5] Chamfer forward (sort, boxes, exact search,
 * reduction), [6] surface sampling forward / backward + Chamfer backward, [7] vertex-feature encoders, image pooling and the
 * image pyramid's library kernels (forward and backward), [8] the optimizer step (a3vt_adam_step).  A class's time is the span from the first to the last launch of each call, summed over calls.
 * Returns the number of classes the library keeps. */
int a3vt_profile_read_classes(double *total_ms, int *count, int n);

#ifdef __cplusplus
}
#endif
#endif /* A3VT_H */
