// capi.hip — extern "C" entry points declared in include/a3vt.h, plus the GCN stack orchestration
// (the layer loop of reconstruction/vision/model.py:316-331 lives here so that Python makes one call
// per refinement stage and nothing syncs the host).
#include <limits.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/a3vt.h"
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <unordered_map>

#include "kernels.h"
#include "prims.h"

namespace a3vt {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- the argument-check vocabulary of the entry points: each returns 0, or -1 with the message set.
// A table of pointer arguments, checked in table order, per entry null first, then alignment.
struct PtrArg {
  const char *name;
  const void *p;
  bool required;
  unsigned align;
  const char *why;
};
static int check_ptrs(const char *who, std::initializer_list<PtrArg> ptrs) {
  for (const PtrArg &a : ptrs) {
    if (a.required && !a.p) {
      set_error("%s: %s=NULL: %s", who, a.name, a.why);
      return -1;
    }
    if (!aligned_to(a.p, a.align)) {
      set_error("%s: %s=%p is not %u-byte aligned", who, a.name, a.p, a.align);
      return -1;
    }
  }
  return 0;
}
// One value against its closed range.
static int check_range(const char *who, const char *name, long long v, long long lo, long long hi) {
  if (v >= lo && v <= hi) return 0;
  set_error("%s: %s=%lld outside %lld..%lld", who, name, v, lo, hi);
  return -1;
}
// One count (rows, steps, a batch, actions) against the largest the kernels take.
static int check_count(const char *who, const char *name, int v, int max) {
  if (v >= 1 && v <= max) return 0;
  set_error("%s: %s=%d (1..%d) unsupported", who, name, v, max);
  return -1;
}
// The gradient table of a layer table of n_layers layers.
static int check_grads(const char *who, const PolicyGrads &g, int n_layers) {
  for (int l = 0; l < n_layers; ++l) {
    if (!g.dw[l] || !g.db[l] || !aligned_to(g.dw[l], 4) || !aligned_to(g.db[l], 4)) {
      set_error("%s: layer %d dweight / dbias null or misaligned", who, l);
      return -1;
    }
  }
  return 0;
}
// Launch counters of a feature's entry points (the a3vt_*_launches test hooks): one relaxed add per accepted call.
template <int N>
struct LaunchCounts {
  std::atomic<long long> n[N];
  void add(int i, long long k) { n[i].fetch_add(k, std::memory_order_relaxed); }
  int read(long long *counts, int reset) {
    for (int i = 0; i < N; ++i) {
      if (counts) counts[i] = n[i].load(std::memory_order_relaxed);
      if (reset) n[i].store(0, std::memory_order_relaxed);
    }
    return N;
  }
};

// 256 bytes of zeros in the code object: source for out-of-range LDS-DMA lanes.
__device__ float g_zero_page[64];
static const float *zero_page() {  // the symbol has one address per device
  static const float *ptr[64] = {};
  static std::mutex mu;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  const float *&slot = ptr[dev & 63];
  if (!slot) {
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_zero_page)) != hipSuccess) return nullptr;
    slot = static_cast<const float *>(p);
  }
  return slot;
}

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump allocator of the scratch layouts below: float offsets, every region 64 floats (256 B) aligned
struct Arena {
  size_t off = 0;
  size_t take(size_t nfloats) {
    const size_t o = off;
    off = align_up(off + nfloats, 64);
    return o;
  }
  size_t take16(size_t nelems) { return take((nelems + 1) / 2 + 64); }   // bf16 region (+ slack for 16-byte tails)
};

// ---- optional per-kernel-class timing with HIP events on the launch stream (bench.py's roofline leg).
// Off by default; when on, every MFMA launch of the GCN stack is bracketed by an event pair.
enum { PROF_GEMM_FWD = 0, PROF_GEMM_DX = 1, PROF_DW = 2, PROF_AGG = 3, PROF_OUT = 4, PROF_SEARCH = 5, PROF_LOSS = 6, PROF_ENC = 7,
       PROF_OPT = 8, PROF_CLASSES = 9 };   // a3vt_profile_read: the first three; a3vt_profile_read_classes: all
struct Prof {
  bool on = false;
  static constexpr int kMax = 8192;
  hipEvent_t ev[kMax][2];
  int cls[kMax];
  int created = 0, used = 0;
};
static Prof g_prof;

struct ProfScope {
  int slot = -1;
  hipStream_t s;
  ProfScope(int cls, hipStream_t stream, bool timed = true) : s(stream) {
    if (!timed || !g_prof.on || g_prof.used >= Prof::kMax) return;
    slot = g_prof.used++;
    if (slot >= g_prof.created) {
      (void)hipEventCreate(&g_prof.ev[slot][0]);
      (void)hipEventCreate(&g_prof.ev[slot][1]);
      g_prof.created = slot + 1;
    }
    g_prof.cls[slot] = cls;
    (void)hipEventRecord(g_prof.ev[slot][0], s);
  }
  ~ProfScope() {
    if (slot >= 0) (void)hipEventRecord(g_prof.ev[slot][1], s);
  }
};

// Scratch layout of a GCN stack call (float offsets, every region 256-B aligned).
struct StackLayout {
  size_t wt, wt_stride;  // per hidden layer: transposed (fwd) or padded (bwd) weight image
  size_t za;             // [M][ldza]
  int ldza;              // row stride of za and gq: cpad, or 4 (dummy rows) without aggregated channels
  size_t z3;             // [2][M][4]
  size_t ping[2];        // [M][hidden] each (fwd without acts: layer outputs; bwd: gradients)
  size_t panel;          // bwd, inputs wider than 304 columns only: [M][300] contiguous column block of X_0 for dW_0
  size_t dw_slab, db_slab, thin_dw_slab, thin_db_slab;
  size_t db_layer_stride;   // db_slab: one block of bias-partial rows per hidden layer
  size_t heavy;          // int32 list of hub rows (csr_heavy_scratch_ints)
  size_t gq;             // bwd: quad-major gradient columns [0, cpad) for the channel-sliced aggregation, [M][ldza]
  size_t ell;            // slot-major index image of the adjacency (csrq_ell_ints)
  size_t total;
};

// Channel-sliced aggregation (gcn_csr.hip "csrq") for the hidden layers of a stack: the mesh slice must fit LDS and the
// product kernel must run the shape as one column block so that its epilogues can write quad-major.  The forward decides
// and records the decision with the stash (stash_layout_*); the backward follows the record.  a3vt_dbg_csr_algo() is the
// test hook that forces either path (both give the same outputs; the shipped library reads no environment variable).
constexpr int kQuadCols = 160;   // quad-major columns of a hybrid layer output: the first column group of rowgemm's epilogue
static std::atomic<long long> g_path_counts[PATH_COUNT];
void path_count(int which) { g_path_counts[which].fetch_add(1, std::memory_order_relaxed); }
static int g_csr_algo = 0;       // 0 = by shape, 1 = half-wave ("rows"), 2 = channel-sliced where it fits, long rows included
static SplitRef split_ref(const a3vt_adj_split *sp) {
  return sp ? SplitRef{sp->rowptr, sp->col, sp->scale, sp->cls} : SplitRef{nullptr, nullptr, nullptr, nullptr};
}
// A split comes whole or not at all (include/a3vt.h).  The stack entry points refuse anything else before they launch, so
// that behind them `split != nullptr` means all four arrays are there.
static bool split_whole(const a3vt_adj_split *sp) {
  const SplitRef r = split_ref(sp);
  return !sp || (r.rowptr && r.col && r.scale && r.cls);
}
// A split the channel-sliced kernels of gcn_csrqs.hip take (P short enough for the slots a thread keeps)
static bool split_usable(const a3vt_adj_split *sp, int n_vert, int cut_len) {
  return sp && sp->max_degree > 0 && sp->max_degree <= csrqs_max_degree() && csrqs_fits(n_vert, cut_len);
}
static bool use_csrq(int batch, int n_vert, int hidden, int cut_len, int mode, int max_degree) {
  // the bf16 operand / storage modes keep the half-wave kernels (GEMM_FP32X3 stores fp32: as GEMM_FP32)
  if (mode == GEMM_BF16_OPERANDS || mode == GEMM_BF16_STORAGE) return false;
  // Rows longer than the eight index slots a thread keeps in registers fall back to per-lane CSR walks: on the fused
  // vision + touch graphs (mean degree 12-26, hub rows of ~1150) that made the step 108 ms where the half-wave kernels
  // take 64 — those graphs stay on the half-wave kernels unless the test hook forces them (they are correct, just slow).
  if (g_csr_algo != 2 && (max_degree <= 0 || max_degree > csrq_max_degree())) return false;
  if (g_csr_algo == 1 || cut_len <= 0) return false;
  return hidden % 4 == 0 && hidden >= kQuadCols + 16 && csrq_fits(n_vert, cut_len) && dw_quad_major_ok(hidden, kQuadCols / 4) &&
         rowgemm_quad_major_ok(batch * n_vert, hidden, pad4(cut_len));
}
// Which layout a forward call left in a stash (activations + sign bytes), keyed by the sign-byte pointer: the backward
// call that receives the same stash adopts it instead of re-deriving it from its own max_degree hint (a C-ABI caller
// that passes csr_max_degree to the forward and csrT_max_degree to the backward would otherwise read hybrid rows as
// row-major ones, silently).  Host-side, a few bytes per live stash; cleared when it grows past 4096 entries.
static std::mutex g_stash_mu;
static std::unordered_map<const void *, int> g_stash_layout;
static void stash_layout_record(const void *masks, bool quad) {
  if (!masks) return;
  std::lock_guard<std::mutex> lock(g_stash_mu);
  if (g_stash_layout.size() > 4096) g_stash_layout.clear();
  g_stash_layout[masks] = quad ? 1 : 0;
}
static int stash_layout_lookup(const void *masks) {   // 1 / 0, or -1 when this library did not write that stash
  std::lock_guard<std::mutex> lock(g_stash_mu);
  auto it = g_stash_layout.find(masks);
  return it == g_stash_layout.end() ? -1 : it->second;
}
// bias gradients of the hidden layers [0, last) from per-layer blocks of partial rows (layer i at slab + i * layer_stride)
static int reduce_bias_partials(const float *slab, size_t layer_stride, int nslab, int cpad, int cut_len, int hidden, int last,
                                float *const *grad_biases, int acc, hipStream_t s) {
  for (int i0 = 0; i0 < last; i0 += kMaxImages) {
    SlabReduceBatch b{};
    b.count = last - i0 < kMaxImages ? last - i0 : kMaxImages;
    b.slab = slab + (size_t)i0 * layer_stride;
    for (int j = 0; j < b.count; ++j) b.out[j] = grad_biases[i0 + j];
    b.layer_stride = layer_stride;
    b.stride = cpad;
    b.n = cut_len;
    b.n_out = hidden;
    b.nslab = nslab;
    b.accumulate = acc;
    if (int rc = launch_slab_reduce_batch(b, s)) return rc;
  }
  return 0;
}

static inline int mask_ld(int hidden, int cut_len) { return pad4(cut_len) / 4 + (hidden + 3) / 4; }

// Hub rows of a CSR (rows longer than csr_heavy_degree()): listed once into `slot`, then every aggregation of the call hands
// them to whole workgroups.  *heavy = NULL when the degree bound rules them out.
static int hub_rows(const int32_t *rowptr, int n_vert, int max_degree, float *slot, int32_t **heavy, hipStream_t s) {
  *heavy = nullptr;
  if (max_degree > 0 && max_degree <= csr_heavy_degree()) return 0;
  *heavy = reinterpret_cast<int32_t *>(slot);
  return launch_csr_heavy_list(rowptr, n_vert, *heavy, s);
}

// Weight images of the layers [i0, i1) of a stack, image i at dst + i * stride, up to kMaxImages layers per launch.
// transpose = 1 (forward): W_i^T as [rowgemm_bt_rows(hidden)][ld of the layer's input]; transpose = 0 (backward): W_i zero
// padded as [rowgemm_bt_rows(width of dX_i)][ld of hidden].  w0 / wh: the row widths of layer 0 / of the hidden layers on
// that side.  kind: GEMM_FP32 (fp32 images: modes 0 and 1, and layer 0 of mode 3), GEMM_BF16_STORAGE (bf16 images, widths
// in bf16) or GEMM_FP32X3 (three bf16 images per layer; hidden layers only).
static int launch_stack_images(int kind, int transpose, const float *const *weights, int i0, int i1, int in_features,
                               int hidden, int w0, int wh, float *dst, size_t stride, hipStream_t s) {
  auto ld = [&](int w) { return kind == GEMM_BF16_STORAGE ? 2 * pad16(w / 2) : pad16(w); };
  for (; i0 < i1; i0 += kMaxImages) {
    WeightImages wi{};
    wi.count = i1 - i0 < kMaxImages ? i1 - i0 : kMaxImages;
    wi.dst = dst + stride * i0;
    wi.dst_stride = stride;
    wi.n = hidden;
    wi.transpose = transpose;
    int max_rows = 0, max_ld = kind == GEMM_FP32 && transpose ? ld(wh) : 0;   // (the fp32 forward grid spans the hidden width)
    for (int j = 0; j < wi.count; ++j) {
      const int w = i0 + j == 0 ? w0 : wh;
      wi.w[j] = weights[i0 + j];
      wi.k[j] = i0 + j == 0 ? in_features : hidden;
      wi.rows[j] = rowgemm_bt_rows(transpose ? hidden : w);
      wi.ld[j] = ld(transpose ? w : wh);
      max_rows = wi.rows[j] > max_rows ? wi.rows[j] : max_rows;
      max_ld = wi.ld[j] > max_ld ? wi.ld[j] : max_ld;
    }
    const int rc = kind == GEMM_FP32X3 ? launch_weight_images3(wi, s)
                   : kind == GEMM_BF16_STORAGE ? launch_weight_images16(wi, max_rows, max_ld, s)
                                               : launch_weight_images(wi, max_rows, max_ld, s);
    if (rc) return rc;
  }
  return 0;
}

// dW / db of the output layer (k inputs, 3 outputs) from the thin kernels' partial slabs
static int reduce_output_grads(const float *dw_slab, const float *db_slab, int k, float *grad_w, float *grad_b, int acc,
                               hipStream_t s) {
  const size_t n = (size_t)k * 3;
  if (int rc = launch_slab_reduce_za(dw_slab, thin_num_slabs(), n, n, n, grad_w, acc, s)) return rc;
  return launch_slab_reduce_za(db_slab, thin_num_slabs(), 3, 3, 3, grad_b, acc, s);
}

// The path decisions of a stack call in modes 0, 1 and 3.  The forward and the backward both take them from here: they
// must agree on the weight images and on the layout of the activations in the stash.
//   Layer outputs are row-major [M][hidden] on the half-wave path.  On the channel-sliced path ("hybrid" rows) the block of
// M * hidden floats holds columns [0, 160) quad-major [batch][40][n_vert] float4 — the aggregated channels written by the
// aggregation kernel, the rest of the product kernel's first column group by its epilogue — followed by columns
// [160, hidden) row-major [M][hidden - 160].  160 = ten 16-column tiles = the input tiles of two waves of dw_kernel and
// ten whole K chunks of rowgemm_kernel: no tile or chunk straddles the two parts.  Every consumer reads either.
struct StackPlan {
  bool x3;        // mode 3: the products of hidden layers 1 .. L-2 on the split-operand kernels (gcn_gemm3.hip)
  int omode;      // operand mode of every other product (the first layer, narrow or short stacks)
  bool quad;      // hidden layers on the channel-sliced aggregation: hybrid rows
  bool qsplit;    // ... through the split (a3vt_adj_split) rather than the CSR
  int qcols;      // columns of a layer's output kept quad-major
  int rm_ld;      // row stride of the row-major part
  size_t rm_off;  // its offset inside a layer's block
};
// rec: the layout recorded with the stash (stash_layout_lookup: 1 / 0), or -1 to decide by shape
static StackPlan stack_plan(int mode, int batch, int n_vert, int hidden, int num_layers, int cut_len, int max_degree,
                            const a3vt_adj_split *split, int rec) {
  StackPlan p{};
  const size_t m = (size_t)batch * n_vert;
  p.x3 = mode == GEMM_FP32X3 && num_layers > 2 && rowgemm3_stack_ok((long long)m, hidden, mask_ld(hidden, cut_len));
  p.omode = mode == GEMM_BF16_OPERANDS ? GEMM_BF16_OPERANDS : GEMM_FP32;
  // a usable split stands for "every row short": the hub and seam rows are gone from P
  const bool split_ok = split_usable(split, n_vert, cut_len);
  p.quad = num_layers > 1 &&
           (rec >= 0 ? rec == 1 : use_csrq(batch, n_vert, hidden, cut_len, mode, split_ok ? csrq_max_degree() : max_degree));
  p.qsplit = p.quad && split_ok;   // P and J are symmetric: the same image serves A^T
  p.qcols = p.quad ? kQuadCols : 0;
  p.rm_ld = hidden - p.qcols;
  p.rm_off = m * p.qcols;
  return p;
}

// The slot-major index image of the channel-sliced aggregation (none on the half-wave path): from the split when the plan
// takes it, from the CSR otherwise
static int launch_stack_ell(const StackPlan &p, const a3vt_adj_split *split, const int32_t *rowptr, const int32_t *col,
                            const float *val, int n_vert, int32_t *ell, hipStream_t s) {
  if (p.qsplit) {
    const SplitRef r = split_ref(split);
    return launch_csrqs_image(r.rowptr, r.col, r.scale, r.cls, n_vert, ell, s);
  }
  return p.quad ? launch_csrq_ell(rowptr, col, val, n_vert, ell, s) : 0;
}

static StackLayout stack_layout(int batch, int n_vert, int in_features, int hidden, int num_layers, int cut_len,
                                int need_backward, int gemm_mode = 0) {
  StackLayout L{};
  const size_t m = (size_t)batch * n_vert;
  const int cpad = pad4(cut_len);
  Arena a;
  const int kmax = hidden > pad4(in_features) ? hidden : pad4(in_features);
  L.wt_stride = align_up((size_t)rowgemm_bt_rows(kmax) * pad16(kmax), 64);
  if (gemm_mode == GEMM_FP32X3 && L.wt_stride < 3 * (size_t)kX3ImageFloats) L.wt_stride = 3 * (size_t)kX3ImageFloats;   // hi / mid / lo images (gcn_gemm3.hip)
  L.wt = a.take(L.wt_stride * (num_layers > 1 ? num_layers - 1 : 1));
  L.ldza = cpad > 4 ? cpad : 4;
  L.za = a.take(m * L.ldza);
  L.z3 = a.take(2 * m * 4);
  L.ping[0] = a.take(m * hidden);
  L.ping[1] = a.take(m * hidden);
  L.heavy = a.take(csr_heavy_scratch_ints(n_vert));
  L.ell = a.take(csrq_ell_ints(n_vert));
  if (need_backward) {
    const size_t kin = kmax;
    // its own region: with hidden < 300 a ping buffer ([M][hidden]) is smaller than a 300-column block of X_0
    L.panel = a.take(pad4(in_features) > 304 ? m * 300 : 0);
    L.dw_slab = a.take((size_t)dw_slab_capacity(hidden) * kin * hidden);
    const size_t nslab = (size_t)csr_bwd_num_slabs(batch, n_vert) > (size_t)batch ? csr_bwd_num_slabs(batch, n_vert) : batch;
    // one block of partial rows PER LAYER ([batch][cpad] on the channel-sliced path, [row-walk workgroups][cpad] otherwise:
    // the stride holds either), reduced by one launch at the end of the backward
    L.db_layer_stride = align_up(nslab * cpad, 64);
    L.db_slab = a.take(L.db_layer_stride * (num_layers > 1 ? num_layers - 1 : 1));
    L.gq = a.take(m * L.ldza);
    L.thin_dw_slab = a.take((size_t)thin_num_slabs() * kin * 3);
    L.thin_db_slab = a.take((size_t)thin_num_slabs() * 3);
  }
  L.total = a.off;
  return L;
}

// dW = X^T dZ of one layer into grad [kin][d.n_out] (+= when acc).  `d` comes filled in except for x, ldx and k_in; x, ldx:
// the layer's input rows.  The kernel covers up to 304 input channels per pass; wider inputs (the 448-wide image model's
// first layer) go in column blocks of <= 300, each first copied into the contiguous `panel` ([M][300]).  Up to 304 channels
// are ONE pass: only the panels start at column c0 (a second pass over 301..304 channels would read X from column 0).
// Hybrid rows (d.xq_nvert > 0) are never wider than that; their ldx is the width of the staged image.
static int dw_panels(DwArgs d, const float *x, int ldx, int kin, float *panel, float *grad, int acc, bool timed, hipStream_t s) {
  const int cblk = kin > 304 ? 300 : kin;
  for (int c0 = 0; c0 < kin; c0 += cblk) {
    const int w = kin - c0 < cblk ? kin - c0 : cblk;
    d.x = x;
    d.ldx = ldx;
    if (kin > 304) {
      // (the stack's own check: check_layer_dims refuses such a width before a3vt_gcn_layer_bwd gets here)
      if (pad4(w) != w) { set_error("gcn_stack: in_features=%d needs a multiple of 4 past 300", kin); return -1; }
      if (int rc = launch_copy_cols(x, ldx, c0, w, panel, (long long)d.m, s)) return rc;
      d.x = panel;
      d.ldx = w;
    }
    d.k_in = w;
    {
      ProfScope ps(PROF_DW, s, timed);
      if (int rc = launch_dw(d, s)) return rc;
    }
    const size_t n = (size_t)w * d.n_out;
    if (int rc = launch_slab_reduce_za(d.slab, dw_images(d), n, n, n, grad + (size_t)c0 * d.n_out, acc, s)) return rc;
  }
  return 0;
}

static int check_stack_dims(int ld_feats, int in_features, int num_layers, int hidden, int cut_len) {
  if (num_layers < 1) { set_error("gcn_stack: num_layers=%d", num_layers); return -1; }
  // the scratch layout (weight-image stride, dW slabs) is sized from in_features alone: the row stride must be the
  // 4-float granule right above it, nothing wider
  if (ld_feats != pad4(in_features)) {
    set_error("gcn_stack: ld_feats=%d must be in_features=%d rounded up to a multiple of 4", ld_feats, in_features);
    return -1;
  }
  if (num_layers > 1 && (hidden % 4 != 0 || hidden > 304 || cut_len < 0 || cut_len > hidden)) {
    set_error("gcn_stack: hidden=%d (must be a multiple of 4, <= 304) cut_len=%d unsupported", hidden, cut_len);
    return -1;
  }
  if (ld_feats > 600) { set_error("gcn_stack: in_features=%d > 600 unsupported", in_features); return -1; }
  if (num_layers == 1 && ld_feats > 320) { set_error("gcn_stack: single-layer stack with %d inputs unsupported", in_features); return -1; }
  return 0;
}


// ---- bf16 STORAGE mode (GEMM_BF16_STORAGE): scratch layout and the stack loops on the bf16 kernels (gcn_bf16s.hip) ----------
// ReLU-sign bytes per row in this mode: the aggregated-channel bytes cover pad8(cut_len) columns, and the row length is
// even so that the 2-byte groups of an 8-column epilogue store never straddle rows
static inline int mask_ld16(int hidden, int cut_len) { return (pad8(cut_len) / 4 + (hidden + 3) / 4 + 1) & ~1; }

constexpr int kStashInputLd = 608;   // pad8 of the widest stack input (check_stack16_dims: in_features <= 600)

// The stash of a stack call: what the forward leaves in the caller's `acts` and `masks` buffers for the backward.  The size
// queries, the forward and the backward of every mode take their offsets from here.
//   acts   modes 0, 1, 3: fp32 rows [M][hidden] per hidden layer (row-major or hybrid: StackPlan).  Mode 2: bf16 rows
//          [M][pad8(hidden)] per hidden layer, then the stack's INPUT rows in bf16 (the backward needs them for dW_0 and would
//          otherwise convert the fp32 features a second time): addressed with row stride pad8(in_features), reserved for the
//          widest input a stack accepts, + slack for 16-byte reads of the last row's tail.
//   masks  row-major ReLU-sign bytes [pad32(M)][mld] per hidden layer; modes 0, 1, 3: behind ALL of them the sign bytes of the
//          aggregated channels, quad-major [batch][pad4(cut_len) / 4][n_vert] per hidden layer (channel-sliced aggregation).
struct StackStash {
  size_t act_stride;           // a layer's rows in `acts`: floats, or bf16 elements in mode 2
  size_t input16;              // mode 2: where the bf16 input rows start (bf16 elements)
  int mld;                     // sign bytes per row (the kernels' mld argument)
  size_t sign_stride;          // a layer's row-major sign bytes
  size_t signq0, signq_stride; // the quad-major sign planes: start, bytes per layer
  size_t acts_bytes, mask_bytes;
  size_t act(int i) const { return (size_t)i * act_stride; }
  size_t signs(int i) const { return (size_t)i * sign_stride; }
  size_t signq(int i) const { return signq0 + (size_t)i * signq_stride; }
};
static StackStash stack_stash(int batch, int n_vert, int hidden, int num_layers, int cut_len, int gemm_mode) {
  StackStash S{};
  const bool s16 = gemm_mode == GEMM_BF16_STORAGE;
  const size_t m = (size_t)batch * n_vert, mpad = (m + 31) / 32 * 32, nh = num_layers > 1 ? num_layers - 1 : 0;
  S.act_stride = m * (s16 ? pad8(hidden) : hidden);
  S.input16 = nh * S.act_stride;
  S.mld = s16 ? mask_ld16(hidden, cut_len) : mask_ld(hidden, cut_len);
  S.sign_stride = mpad * S.mld;
  S.signq0 = nh * S.sign_stride;
  S.signq_stride = s16 ? 0 : align_up(m * (size_t)(pad4(cut_len) / 4), 256);
  S.acts_bytes = s16 ? (S.input16 + m * (size_t)kStashInputLd) * 2 + 256 : nh * S.act_stride * sizeof(float);
  S.mask_bytes = nh * (S.sign_stride + S.signq_stride);
  return S;
}
struct Stack16Layout {
  size_t wt, wt_stride;   // bf16 weight images (offsets / stride in floats)
  size_t feats16;         // [M][ld0] bf16: the stack's fp32 input features, converted
  size_t za;              // [M][ldza] bf16
  size_t z3;              // [2][M][4] fp32
  size_t ping[2];         // [M][ldh] bf16 each
  size_t dw_slab, db_slab, thin_dw_slab, thin_db_slab, heavy, total;
  size_t db_layer_stride; // db_slab: one block of bias-partial rows per hidden layer
  size_t tplan;           // the tiled aggregation's plan (csr16t_plan_ints)
  int ld0, ldh, cpad;
  int ldza;               // row stride of za: cpad, at least one 8-column group
};

static Stack16Layout stack16_layout(int batch, int n_vert, int in_features, int hidden, int num_layers, int cut_len,
                                    int need_backward) {
  Stack16Layout L{};
  const size_t m = (size_t)batch * n_vert;
  L.ld0 = pad8(in_features);
  L.ldh = pad8(hidden);
  L.cpad = pad8(cut_len);
  L.ldza = L.cpad > 8 ? L.cpad : 8;
  Arena a;
  // images: forward W_i^T [bt_rows(hidden)][2 pad16(k_i / 2)], backward W_i [bt_rows(n_store_i)][2 pad16(ldh / 2)]
  const int kmax = L.ld0 > L.ldh ? L.ld0 : L.ldh;
  const int rows_f = rowgemm_bt_rows(hidden), rows_b = rowgemm_bt_rows(kmax);
  const size_t img_f = (size_t)rows_f * pad16(kmax / 2), img_b = (size_t)rows_b * pad16(L.ldh / 2);
  L.wt_stride = align_up(img_f > img_b ? img_f : img_b, 64);
  L.wt = a.take(L.wt_stride * (num_layers > 1 ? num_layers - 1 : 1));
  L.feats16 = a.take16(m * L.ld0);
  L.za = a.take16(m * L.ldza);
  L.z3 = a.take(2 * m * 4);
  L.ping[0] = a.take16(m * L.ldh);
  L.ping[1] = a.take16(m * L.ldh);
  L.heavy = a.take(csr_heavy_scratch_ints(n_vert));
  L.tplan = a.take(csr16t_plan_ints(n_vert));
  if (need_backward) {
    const size_t kin = in_features > hidden ? in_features : hidden;
    L.dw_slab = a.take((size_t)dw16_num_slabs(hidden) * (kin > 304 ? 304 : kin) * hidden);
    L.db_layer_stride = align_up((size_t)csr_bwd_num_slabs(batch, n_vert) * L.ldza, 64);
    L.db_slab = a.take(L.db_layer_stride * (num_layers > 1 ? num_layers - 1 : 1));
    L.thin_dw_slab = a.take((size_t)thin_num_slabs() * hidden * 3);
    L.thin_db_slab = a.take((size_t)thin_num_slabs() * 3);
  }
  L.total = a.off;
  return L;
}

static int check_stack16_dims(int num_layers, int hidden, int in_features) {
  if (num_layers < 2) { set_error("gcn_stack: the bf16 storage mode needs at least one hidden layer"); return -1; }
  if (num_layers - 1 > kMaxImages) { set_error("gcn_stack: bf16 storage mode supports up to %d hidden layers", kMaxImages); return -1; }
  if (hidden > 304 || hidden % 4 != 0 || hidden < 16) { set_error("gcn_stack: bf16 storage mode: hidden=%d unsupported", hidden); return -1; }
  if (in_features > 600) { set_error("gcn_stack: in_features=%d > 600 unsupported", in_features); return -1; }
  if (in_features > 304 && in_features % 8 != 0) {
    set_error("gcn_stack: bf16 storage mode: in_features=%d > 304 must be a multiple of 8", in_features);
    return -1;
  }
  return 0;
}

static int stack_fwd16(const float *feats, int ld_feats, int in_features, const float *const *weights,
                       const float *const *biases, int num_layers, int hidden, int cut_len, const int32_t *rowptr,
                       const int32_t *col, const float *val, int max_degree, const a3vt_adj_split *split, int n_vert,
                       int batch, void *acts, uint8_t *masks, float *scratch, float *update, hipStream_t s) {
  if (int rc = check_stack16_dims(num_layers, hidden, in_features)) return rc;
  const float *zeros = zero_page();
  A3VT_CHECK_ARG(zeros != nullptr);
  const Stack16Layout L = stack16_layout(batch, n_vert, in_features, hidden, num_layers, cut_len, 0);
  const StackStash S = stack_stash(batch, n_vert, hidden, num_layers, cut_len, GEMM_BF16_STORAGE);
  const size_t m = (size_t)batch * n_vert;
  int32_t *heavy;
  if (int rc = hub_rows(rowptr, n_vert, max_degree, scratch + L.heavy, &heavy, s)) return rc;
  if (int rc = launch_stack_images(GEMM_BF16_STORAGE, 1, weights, 0, num_layers - 1, in_features, hidden, L.ld0, L.ldh,
                                   scratch + L.wt, L.wt_stride, s))
    return rc;
  // the input rows in bf16: behind the hidden layers' rows in the stash when there is one (the backward reads them there)
  u16 *f16 = acts ? static_cast<u16 *>(acts) + S.input16 : reinterpret_cast<u16 *>(scratch + L.feats16);
  if (int rc = launch_cvt_rows(feats, ld_feats, in_features, f16, L.ld0, (long long)m, s)) return rc;
  // bounded-degree graphs: the aggregation reads its neighbour rows from LDS tiles (gcn_bf16s.hip, csr16t); plan per call
  const bool tiled = heavy == nullptr && cut_len > 0 && g_csr_algo != 1 && csr16t_ok(n_vert, cut_len, max_degree, (long long)m);
  int32_t *tplan = reinterpret_cast<int32_t *>(scratch + L.tplan);
  if (tiled)
    if (int rc = launch_csr16t_build(rowptr, col, val, n_vert, tplan, s)) return rc;

  const u16 *x = f16;
  int ldx = L.ld0;
  u16 *za = reinterpret_cast<u16 *>(scratch + L.za);
  for (int i = 0; i + 1 < num_layers; ++i) {
    u16 *y = acts ? static_cast<u16 *>(acts) + S.act(i) : reinterpret_cast<u16 *>(scratch + L.ping[i & 1]);
    RowGemmArgs g{};
    g.a0 = g.a1 = reinterpret_cast<const float *>(x);
    g.lda0 = g.lda1 = ldx / 2;
    g.ksplit = g.k = ldx / 2;
    g.bt = scratch + L.wt + L.wt_stride * i;
    g.ldb = pad16(ldx / 2);
    g.zeros = zeros;
    g.m = (int)m;
    g.n_store = hidden;
    g.c = reinterpret_cast<float *>(y);
    g.ldc = L.ldh;
    g.c2 = reinterpret_cast<float *>(za);
    g.ldc2 = L.ldza;
    g.csplit = cut_len;
    uint8_t *mk = masks ? masks + S.signs(i) : nullptr;
    g.maskb = mk;
    g.mld = S.mld;
    g.moff = L.cpad / 4;
    g.mode = GEMM_BF16_STORAGE;
    {
      ProfScope ps(PROF_GEMM_FWD, s);
      if (int rc = launch_rowgemm(g, EPI_FWD_HIDDEN, s)) return rc;
    }
    if (cut_len > 0) {
      ProfScope psa(PROF_AGG, s);
      if (tiled) {
        if (int rc = launch_csr16t_fwd(za, g.ldc2, biases[i], cut_len, tplan, rowptr, col, val, n_vert, batch, y, L.ldh, mk, S.mld, 1, s))
          return rc;
      } else if (int rc = launch_csr16_fwd(za, g.ldc2, biases[i], cut_len, rowptr, col, val, heavy, n_vert, batch, y, L.ldh, mk, S.mld, 1, s)) {
        return rc;
      }
    }
    x = y;
    ldx = L.ldh;
  }
  const int last = num_layers - 1;
  ProfScope pso(PROF_OUT, s);
  if (int rc = launch_thin16_fwd_product(x, ldx, hidden, weights[last], (long long)m, scratch + L.z3, s)) return rc;
  const SplitRef sref = split_ref(split);
  return launch_csr3(scratch + L.z3, biases[last], rowptr, col, val, heavy, n_vert, batch, update, 3, s, split ? &sref : nullptr,
                     false);
}

static int stack_bwd16(const float *feats, int ld_feats, int in_features, const float *const *weights, int num_layers,
                       int hidden, int cut_len, const int32_t *rowptrT, const int32_t *colT, const float *valT,
                       int max_degreeT, const a3vt_adj_split *split, int n_vert, int batch, const void *acts,
                       const uint8_t *masks, const float *grad_update, float *const *grad_weights,
                       float *const *grad_biases, float *grad_feats, float *scratch, int acc, hipStream_t s) {
  if (int rc = check_stack16_dims(num_layers, hidden, in_features)) return rc;
  const float *zeros = zero_page();
  A3VT_CHECK_ARG(zeros != nullptr);
  const Stack16Layout L = stack16_layout(batch, n_vert, in_features, hidden, num_layers, cut_len, 1);
  const StackStash S = stack_stash(batch, n_vert, hidden, num_layers, cut_len, GEMM_BF16_STORAGE);
  const size_t m = (size_t)batch * n_vert;
  const int last = num_layers - 1;
  const u16 *acts16 = static_cast<const u16 *>(acts);
  int32_t *heavyT;
  if (int rc = hub_rows(rowptrT, n_vert, max_degreeT, scratch + L.heavy, &heavyT, s)) return rc;
  // the stack's input in bf16: the forward left it behind the hidden layers' rows in the stash (StackStash)
  const u16 *f16 = acts16 + S.input16;
  (void)feats;
  (void)ld_feats;
  // the tiled aggregation's plan for A^T (see stack_fwd16)
  const bool tiled = heavyT == nullptr && cut_len > 0 && g_csr_algo != 1 && csr16t_ok(n_vert, cut_len, max_degreeT, (long long)m);
  int32_t *tplan = reinterpret_cast<int32_t *>(scratch + L.tplan);
  if (tiled)
    if (int rc = launch_csr16t_build(rowptrT, colT, valT, n_vert, tplan, s)) return rc;

  // ---- output layer: dz3 = A^T dU, then one pass over X_{L-1}: G (bf16, ReLU-masked), dW, db partials
  u16 *ping[2] = {reinterpret_cast<u16 *>(scratch + L.ping[0]), reinterpret_cast<u16 *>(scratch + L.ping[1])};
  {
    float *du4 = scratch + L.z3, *res = scratch + L.z3 + m * 4;
    ProfScope pso(PROF_OUT, s);
    if (int rc = launch_pad3to4(grad_update, (long long)m, du4, s)) return rc;
    const SplitRef sref = split_ref(split);
    if (int rc = launch_csr3(du4, nullptr, rowptrT, colT, valT, heavyT, n_vert, batch, res, 4, s, split ? &sref : nullptr, true))
      return rc;
    const u16 *x = acts16 + S.act(last - 1);
    if (int rc = launch_thin16_bwd_main(x, L.ldh, hidden, weights[last], res, grad_update, (long long)m, 1, ping[0], L.ldh,
                                        scratch + L.thin_dw_slab, scratch + L.thin_db_slab, s))
      return rc;
    if (int rc = reduce_output_grads(scratch + L.thin_dw_slab, scratch + L.thin_db_slab, hidden, grad_weights[last],
                                     grad_biases[last], acc, s))
      return rc;
  }
  // bf16 images Bt = W_i (zero padded) for dX_i = dZ W_i^T
  if (int rc = launch_stack_images(GEMM_BF16_STORAGE, 0, weights, 0, last, in_features, hidden, ld_feats, L.ldh, scratch + L.wt,
                                   L.wt_stride, s))
    return rc;
  u16 *dza = reinterpret_cast<u16 *>(scratch + L.za);
  const int cpad = L.cpad, ldza = L.ldza;
  int cur = 0;
  for (int i = last - 1; i >= 0; --i) {
    u16 *g = ping[cur];
    const u16 *x = i == 0 ? f16 : acts16 + S.act(i - 1);
    const int ldx = i == 0 ? L.ld0 : L.ldh;
    const int kin = i == 0 ? in_features : hidden;
    if (cut_len > 0) {
      ProfScope psa(PROF_AGG, s);
      if (tiled) {
        if (int rc = launch_csr16t_bwd(g, L.ldh, cut_len, cpad, tplan, rowptrT, colT, valT, n_vert, batch, dza, ldza,
                                       scratch + L.db_slab + (size_t)i * L.db_layer_stride, s))
          return rc;
      } else if (int rc = launch_csr16_bwd(g, L.ldh, cut_len, cpad, rowptrT, colT, valT, heavyT, n_vert, batch, dza, ldza,
                                           scratch + L.db_slab + (size_t)i * L.db_layer_stride, s)) {
        return rc;
      }
    } else if (!acc) {
      if (int rc = launch_fill_zero(grad_biases[i], hidden, s)) return rc;
    }
    // dW_i = X_i^T dZ in panels of <= 304 input channels (windows of the rows: no copies)
    for (int c0 = 0; c0 < kin; c0 += 304) {
      const int w = kin - c0 < 304 ? kin - c0 : 304;
      Dw16Args d{};
      d.x = x;
      d.ldx = ldx;
      d.xc0 = c0;
      d.xw = pad8(w);
      d.z0 = dza;
      d.ldz0 = ldza;
      d.z1 = g;
      d.ldz1 = L.ldh;
      d.zsplit = cut_len > 0 ? cpad : 0;
      d.zeros = zeros;
      d.slab = scratch + L.dw_slab;
      d.m = (int)m;
      d.k_in = w;
      d.n_out = hidden;
      {
        ProfScope ps(PROF_DW, s);
        if (int rc = launch_dw16(d, s)) return rc;
      }
      if (int rc = launch_slab_reduce_za(scratch + L.dw_slab, dw16_num_slabs(hidden), (size_t)w * hidden, (size_t)w * hidden,
                                         (size_t)w * hidden, grad_weights[i] + (size_t)c0 * hidden, acc, s))
        return rc;
    }
    // dX_i = dZ W_i^T
    RowGemmArgs r{};
    r.a0 = reinterpret_cast<const float *>(dza);
    r.lda0 = ldza / 2;
    r.a1 = reinterpret_cast<const float *>(g);
    r.lda1 = L.ldh / 2;
    r.ksplit = cut_len > 0 ? cpad / 2 : 0;
    r.k = L.ldh / 2;
    r.bt = scratch + L.wt + L.wt_stride * i;
    r.ldb = pad16(L.ldh / 2);
    r.zeros = zeros;
    r.m = (int)m;
    r.mode = GEMM_BF16_STORAGE;
    if (i == 0) {
      r.n_store = ld_feats;
      r.c = grad_feats;
      r.ldc = ld_feats;
      if (int rc = launch_rowgemm(r, EPI_PLAIN, s)) return rc;
    } else {
      r.n_store = hidden;
      r.c = reinterpret_cast<float *>(ping[cur ^ 1]);
      r.ldc = L.ldh;
      r.maskb = const_cast<uint8_t *>(masks) + S.signs(i - 1);
      r.mld = S.mld;
      r.moff = cpad / 4;
      r.csplit = cut_len;
      {
        ProfScope ps(PROF_GEMM_DX, s);
        if (int rc = launch_rowgemm(r, EPI_DX_MASK, s)) return rc;
      }
      cur ^= 1;
    }
  }
  if (cut_len > 0)   // bias gradients of all hidden layers: one launch (as the fp32 stack)
    if (int rc = reduce_bias_partials(scratch + L.db_slab, L.db_layer_stride, csr_bwd_num_slabs(batch, n_vert), cpad, cut_len, hidden,
                                      last, grad_biases, acc, s))
      return rc;
  return 0;
}

}  // namespace a3vt

using namespace a3vt;

extern "C" {

int a3vt_version(void) { return A3VT_VERSION; }
const char *a3vt_last_error(void) { return g_err; }

int a3vt_csr_validate(const int32_t *rowptr, const int32_t *col, int n_vert, int nnz) {
  A3VT_CHECK_ARG(rowptr && col && n_vert > 0 && nnz >= 0);
  if (rowptr[0] != 0 || rowptr[n_vert] != nnz) {
    set_error("csr: rowptr[0]=%d rowptr[n]=%d nnz=%d", rowptr[0], rowptr[n_vert], nnz);
    return -1;
  }
  for (int i = 0; i < n_vert; ++i)
    if (rowptr[i + 1] < rowptr[i]) { set_error("csr: rowptr not monotone at %d", i); return -1; }
  for (int e = 0; e < nnz; ++e)
    if (col[e] < 0 || col[e] >= n_vert) { set_error("csr: col[%d]=%d out of range", e, col[e]); return -1; }
  return 0;
}

int a3vt_adj_split_validate(const int32_t *rowptr, const int32_t *col, const float *val, int n_vert,
                            const int32_t *p_rowptr, const int32_t *p_col, const float *scale, const uint8_t *cls) {
  A3VT_CHECK_ARG(rowptr && col && val && p_rowptr && p_col && scale && cls && n_vert > 0);
  // p_rowptr first, whole: the row walks below (and the symmetry search into rows not yet walked) index p_col with it
  if (p_rowptr[0] != 0 || p_rowptr[n_vert] > rowptr[n_vert]) {
    set_error("adj_split: p_rowptr[0]=%d p_rowptr[n]=%d (the matrix has %d entries)", p_rowptr[0], p_rowptr[n_vert], rowptr[n_vert]);
    return -1;
  }
  for (int i = 0; i < n_vert; ++i)
    if (p_rowptr[i + 1] < p_rowptr[i]) { set_error("adj_split: p_rowptr not monotone at %d", i); return -1; }
  // the two classes, ascending
  int ns = 0, nc = 0;
  for (int i = 0; i < n_vert; ++i) {
    if (cls[i] > 2) { set_error("adj_split: cls[%d]=%d", i, (int)cls[i]); return -1; }
    ns += cls[i] == 1;
    nc += cls[i] == 2;
  }
  if ((ns == 0) != (nc == 0)) { set_error("adj_split: %d seam vertices but %d centres", ns, nc); return -1; }
  int32_t *members = static_cast<int32_t *>(malloc(sizeof(int32_t) * (size_t)(ns + nc + 1)));
  A3VT_CHECK_ARG(members != nullptr);
  int32_t *seam = members, *centre = members + ns;
  for (int i = 0, a = 0, b = 0; i < n_vert; ++i) {
    if (cls[i] == 1) seam[a++] = i;
    if (cls[i] == 2) centre[b++] = i;
  }
  int rc = 0;
  for (int i = 0; i < n_vert && rc == 0; ++i) {
    const int e0 = rowptr[i], e1 = rowptr[i + 1], p0 = p_rowptr[i], p1 = p_rowptr[i + 1];
    const int32_t *other = cls[i] == 1 ? centre : cls[i] == 2 ? seam : nullptr;
    const int no = cls[i] == 1 ? nc : cls[i] == 2 ? ns : 0;
    if (p1 < p0 || e1 - e0 != (p1 - p0) + no) {
      set_error("adj_split: row %d has %d entries, the split gives %d + %d", i, e1 - e0, p1 - p0, no);
      rc = -1;
      break;
    }
    // merge of the row of P (ascending, in range, no duplicates) with the other class (ascending): must reproduce the row
    int a = p0, b = 0;
    for (int e = e0; e < e1; ++e) {
      const bool has_a = a < p1, has_b = b < no;
      int next;
      if (has_a && has_b && p_col[a] == other[b]) {
        set_error("adj_split: row %d: column %d is in P and in the bipartite block", i, p_col[a]);
        rc = -1;
        break;
      }
      if (has_a && (!has_b || p_col[a] < other[b])) {
        next = p_col[a++];
        if (next < 0 || next >= n_vert || (a - 1 > p0 && p_col[a - 2] >= next)) {
          set_error("adj_split: row %d of P is not ascending / in range at column %d", i, next);
          rc = -1;
          break;
        }
        // symmetry of P: (next, i) must be an entry of row `next` (binary search)
        int lo = p_rowptr[next], hi = p_rowptr[next + 1] - 1;
        bool found = false;
        while (lo <= hi) {
          const int mid = (lo + hi) / 2;
          if (p_col[mid] == i) { found = true; break; }
          if (p_col[mid] < i) lo = mid + 1;
          else hi = mid - 1;
        }
        if (!found) { set_error("adj_split: P has (%d, %d) but not (%d, %d)", i, next, next, i); rc = -1; break; }
      } else {
        next = other[b++];
      }
      if (col[e] != next) {
        set_error("adj_split: row %d entry %d: column %d, the split gives %d", i, e - e0, col[e], next);
        rc = -1;
        break;
      }
      if (memcmp(&val[e], &scale[i], sizeof(float)) != 0) {
        set_error("adj_split: row %d entry %d: value %.9g != scale %.9g", i, e - e0, (double)val[e], (double)scale[i]);
        rc = -1;
        break;
      }
    }
  }
  free(members);
  return rc;
}

// ReLU-sign bytes saved by the forward pass for the backward pass in modes 0, 1 and 3 (StackStash)
size_t a3vt_gcn_stack_mask_bytes(int batch, int n_vert, int hidden, int num_layers, int cut_len) {
  if (num_layers < 2 || batch <= 0 || n_vert <= 0 || hidden <= 0 || cut_len < 0) return 0;
  return stack_stash(batch, n_vert, hidden, num_layers, cut_len, GEMM_FP32).mask_bytes;
}

size_t a3vt_gcn_stack_scratch_bytes(int batch, int n_vert, int in_features, int hidden, int num_layers, int cut_len,
                                    int need_backward) {
  // enough for EVERY gemm mode (mode 3 keeps three bf16 images per hidden layer: a larger weight slot than mode 0's;
  // mode 2 has a layout of its own): a caller that sizes its scratch here may pass any gemm_bf16
  size_t most = 0;
  for (int mode = 0; mode <= 3; ++mode) {
    if (mode == GEMM_BF16_STORAGE && num_layers < 2) continue;
    const size_t b = a3vt_gcn_stack_scratch_bytes_mode(batch, n_vert, in_features, hidden, num_layers, cut_len, need_backward, mode);
    most = b > most ? b : most;
  }
  return most;
}

size_t a3vt_gcn_stack_scratch_bytes_mode(int batch, int n_vert, int in_features, int hidden, int num_layers,
                                         int cut_len, int need_backward, int gemm_bf16) {
  // (a size query never fails: sizes no stack call accepts give 0 — the layouts below divide by some of them)
  if (batch <= 0 || n_vert <= 0 || in_features <= 0 || hidden <= 0 || num_layers <= 0 || cut_len < 0 || gemm_bf16 < 0 || gemm_bf16 > 3)
    return 0;
  if (gemm_bf16 == GEMM_BF16_STORAGE)
    return stack16_layout(batch, n_vert, in_features, hidden, num_layers, cut_len, need_backward).total * sizeof(float);
  return stack_layout(batch, n_vert, in_features, hidden, num_layers, cut_len, need_backward, gemm_bf16).total * sizeof(float);
}

int a3vt_gcn_stack_stash_bytes(int batch, int n_vert, int hidden, int num_layers, int cut_len, int gemm_bf16,
                               size_t *acts_bytes, size_t *mask_bytes) {
  A3VT_CHECK_ARG(acts_bytes && mask_bytes && batch > 0 && n_vert > 0 && hidden > 0 && cut_len >= 0);
  *acts_bytes = *mask_bytes = 0;
  if (num_layers < 2) return 0;
  const StackStash S = stack_stash(batch, n_vert, hidden, num_layers, cut_len, gemm_bf16);
  *acts_bytes = S.acts_bytes;
  *mask_bytes = S.mask_bytes;
  return 0;
}

int a3vt_gcn_stack_fwd(const float *feats, int ld_feats, int in_features, const float *const *weights,
                       const float *const *biases, int num_layers, int hidden, int cut_len,
                       const int32_t *rowptr, const int32_t *col, const float *val, int max_degree, int n_vert,
                       int batch, int gemm_bf16, void *acts_v, uint8_t *masks, float *scratch, float *update,
                       void *stream) {
  return a3vt_gcn_stack_fwd_adj(feats, ld_feats, in_features, weights, biases, num_layers, hidden, cut_len, rowptr, col, val,
                                max_degree, nullptr, n_vert, batch, gemm_bf16, acts_v, masks, scratch, update, stream);
}

int a3vt_gcn_stack_fwd_adj(const float *feats, int ld_feats, int in_features, const float *const *weights,
                           const float *const *biases, int num_layers, int hidden, int cut_len,
                           const int32_t *rowptr, const int32_t *col, const float *val, int max_degree,
                           const a3vt_adj_split *split, int n_vert,
                           int batch, int gemm_bf16, void *acts_v, uint8_t *masks, float *scratch, float *update,
                           void *stream) {
  float *acts = static_cast<float *>(acts_v);
  A3VT_CHECK_ARG(feats && weights && biases && rowptr && col && val && scratch && update);
  A3VT_CHECK_ARG((acts == nullptr) == (masks == nullptr) || num_layers < 2);
  A3VT_CHECK_ARG(n_vert > 0 && batch > 0 && split_whole(split));
  A3VT_CHECK_ARG(gemm_bf16 >= GEMM_FP32 && gemm_bf16 <= GEMM_FP32X3);
  if (int rc = check_stack_dims(ld_feats, in_features, num_layers, hidden, cut_len)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (gemm_bf16 == GEMM_BF16_STORAGE)  // bf16 storage: `acts` holds bf16 rows (a3vt_gcn_stack_stash_bytes)
    return stack_fwd16(feats, ld_feats, in_features, weights, biases, num_layers, hidden, cut_len, rowptr, col, val,
                       max_degree, split, n_vert, batch, acts, masks, scratch, update, s);
  const float *zeros = zero_page();
  A3VT_CHECK_ARG(zeros != nullptr);
  const StackLayout L = stack_layout(batch, n_vert, in_features, hidden, num_layers, cut_len, 0, gemm_bf16);
  const StackStash S = stack_stash(batch, n_vert, hidden, num_layers, cut_len, gemm_bf16);
  const size_t m = (size_t)batch * n_vert;
  const int cpad = pad4(cut_len);

  int32_t *heavy;
  if (int rc = hub_rows(rowptr, n_vert, max_degree, scratch + L.heavy, &heavy, s)) return rc;
  const StackPlan P = stack_plan(gemm_bf16, batch, n_vert, hidden, num_layers, cut_len, max_degree, split, -1);
  const int qcols = P.qcols, rm_ld = P.rm_ld;
  const size_t rm_off = P.rm_off;
  // transposed, zero-padded weight images of the hidden layers; mode 3: layers 1 .. L-2 as three bf16 images each, layer 0
  // (K = in_features) keeps its fp32 image
  if (P.x3)
    if (int rc = launch_stack_images(GEMM_FP32X3, 1, weights, 1, num_layers - 1, in_features, hidden, ld_feats, hidden,
                                     scratch + L.wt, L.wt_stride, s))
      return rc;
  if (int rc = launch_stack_images(GEMM_FP32, 1, weights, 0, P.x3 ? 1 : num_layers - 1, in_features, hidden, ld_feats, hidden,
                                   scratch + L.wt, L.wt_stride, s))
    return rc;
  if (num_layers > 1) path_count(P.quad ? PATH_STACK_QUAD : PATH_STACK_ROWS);
  if (P.qsplit) path_count(PATH_STACK_SPLIT);
  if (num_layers > 1) stash_layout_record(masks, P.quad);
  int32_t *ell = reinterpret_cast<int32_t *>(scratch + L.ell);
  if (int rc = launch_stack_ell(P, split, rowptr, col, val, n_vert, ell, s)) return rc;
  const float *x = feats, *xq = nullptr;                     // x: pre-offset so that x + row * ldx + col is column col
  int ldx = ld_feats;
  for (int i = 0; i + 1 < num_layers; ++i) {
    const int k = i == 0 ? ld_feats : hidden;       // K walked by the kernel (pad columns of feats are zero)
    const bool l3 = P.x3 && i > 0;   // this layer's product on the split-operand kernel
    float *y = acts ? acts + S.act(i) : scratch + L.ping[i & 1];
    RowGemmArgs g{};
    g.a0 = g.a1 = x;
    g.lda0 = g.lda1 = ldx;
    g.ksplit = k;
    if (xq) {   // hybrid input rows: columns [0, 160) from the quad-major part
      g.a0 = xq;
      g.ksplit = qcols;
      g.a0q_nvert = n_vert;
      g.a0q_quads = qcols / 4;
    }
    g.bt = scratch + L.wt + L.wt_stride * i;
    g.ldb = pad16(k);
    g.zeros = zeros;
    g.m = (int)m;
    g.k = k;
    g.n_store = hidden;
    g.c = y + rm_off - qcols;
    g.ldc = rm_ld;
    g.c2 = scratch + L.za;
    g.ldc2 = cpad;   // (not L.ldza: 0 without aggregated channels, nothing goes to c2 then)
    g.csplit = cut_len;
    uint8_t *mk = masks ? masks + S.signs(i) : nullptr;
    g.maskb = mk;
    g.mld = S.mld;
    g.moff = cpad / 4;
    g.mode = l3 ? GEMM_FP32X3 : P.omode;
    if (P.quad) {   // raw columns [0, cpad) leave the product quad-major, for the channel-sliced aggregation;
      g.zq_nvert = n_vert;   // activated columns [cpad, 160) quad-major into the layer's output
      g.zq_quads = cpad / 4;
      g.yq = y;
      g.yq_quads = qcols / 4;
      g.trash = scratch + L.z3;   // (the output layer's scratch: idle while the hidden layers run)
    }
    {
      ProfScope ps(PROF_GEMM_FWD, s);
      if (int rc = launch_rowgemm(g, EPI_FWD_HIDDEN, s)) return rc;
    }
    if (P.quad) {
      uint8_t *sq = masks ? masks + S.signq(i) : nullptr;
      ProfScope psa(PROF_AGG, s);
      if (P.qsplit) {
        if (int rc = launch_csrqs_fwd(scratch + L.za, biases[i], cut_len, ell, n_vert, batch, y, qcols / 4, sq, 1, s)) return rc;
      } else if (int rc = launch_csrq_fwd(scratch + L.za, biases[i], cut_len, rowptr, col, val, heavy, ell, n_vert, batch, y, qcols / 4, sq, 1, s)) {
        return rc;
      }
      xq = y;
    } else if (cut_len > 0) {
      ProfScope psa(PROF_AGG, s);
      if (int rc = launch_csr_fwd(scratch + L.za, L.ldza, biases[i], cut_len, rowptr, col, val, heavy, n_vert, batch, y, hidden, mk, S.mld, 1, s))
        return rc;
    }
    x = y + rm_off - qcols;
    ldx = rm_ld;
  }
  const int klast = num_layers == 1 ? in_features : hidden;
  ProfScope pso(PROF_OUT, s);
  // the 3-channel aggregation of the output layer through the split (any P: its rows are walked from global memory)
  const SplitRef sref = split_ref(split);
  return launch_thin_fwd(x, ldx, klast, weights[num_layers - 1], biases[num_layers - 1], rowptr, col, val, heavy, n_vert,
                         batch, scratch + L.z3, update, xq, qcols / 4, s, split ? &sref : nullptr);
}

int a3vt_gcn_stack_bwd(const float *feats, int ld_feats, int in_features, const float *const *weights,
                       const float *const *biases, int num_layers, int hidden, int cut_len,
                       const int32_t *rowptr, const int32_t *col, const float *val, const int32_t *rowptrT,
                       const int32_t *colT, const float *valT, int max_degreeT, int n_vert, int batch, int gemm_bf16,
                       const void *acts_v,
                       const uint8_t *masks, const float *grad_update, float *const *grad_weights, float *const *grad_biases,
                       float *grad_feats, float *scratch, void *stream) {
  return a3vt_gcn_stack_bwd_adj(feats, ld_feats, in_features, weights, biases, num_layers, hidden, cut_len, rowptr, col, val,
                                rowptrT, colT, valT, max_degreeT, nullptr, n_vert, batch, gemm_bf16, acts_v, masks, grad_update,
                                grad_weights, grad_biases, grad_feats, scratch, 0, stream);
}

int a3vt_gcn_stack_bwd_acc(const float *feats, int ld_feats, int in_features, const float *const *weights,
                           const float *const *biases, int num_layers, int hidden, int cut_len,
                           const int32_t *rowptr, const int32_t *col, const float *val, const int32_t *rowptrT,
                           const int32_t *colT, const float *valT, int max_degreeT, int n_vert, int batch, int gemm_bf16,
                           const void *acts_v,
                           const uint8_t *masks, const float *grad_update, float *const *grad_weights,
                           float *const *grad_biases, float *grad_feats, float *scratch, int accumulate, void *stream) {
  return a3vt_gcn_stack_bwd_adj(feats, ld_feats, in_features, weights, biases, num_layers, hidden, cut_len, rowptr, col, val,
                                rowptrT, colT, valT, max_degreeT, nullptr, n_vert, batch, gemm_bf16, acts_v, masks, grad_update,
                                grad_weights, grad_biases, grad_feats, scratch, accumulate, stream);
}

int a3vt_gcn_stack_bwd_adj(const float *feats, int ld_feats, int in_features, const float *const *weights,
                           const float *const *biases, int num_layers, int hidden, int cut_len,
                           const int32_t *rowptr, const int32_t *col, const float *val, const int32_t *rowptrT,
                           const int32_t *colT, const float *valT, int max_degreeT, const a3vt_adj_split *split,
                           int n_vert, int batch, int gemm_bf16, const void *acts_v,
                           const uint8_t *masks, const float *grad_update, float *const *grad_weights,
                           float *const *grad_biases, float *grad_feats, float *scratch, int accumulate, void *stream) {
  const int acc = accumulate ? 1 : 0;
  const float *acts = static_cast<const float *>(acts_v);
  (void)biases; (void)rowptr; (void)col; (void)val;
  A3VT_CHECK_ARG(feats && weights && rowptrT && colT && valT && grad_update && grad_weights && grad_biases);
  A3VT_CHECK_ARG(grad_feats && scratch && n_vert > 0 && batch > 0 && split_whole(split));
  A3VT_CHECK_ARG(gemm_bf16 >= GEMM_FP32 && gemm_bf16 <= GEMM_FP32X3);
  A3VT_CHECK_ARG(num_layers == 1 || acts != nullptr);
  A3VT_CHECK_ARG(num_layers <= 2 || masks != nullptr);
  if (int rc = check_stack_dims(ld_feats, in_features, num_layers, hidden, cut_len)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (gemm_bf16 == GEMM_BF16_STORAGE)
    return stack_bwd16(feats, ld_feats, in_features, weights, num_layers, hidden, cut_len, rowptrT, colT, valT,
                       max_degreeT, split, n_vert, batch, acts, masks, grad_update, grad_weights, grad_biases, grad_feats,
                       scratch, acc, s);
  const float *zeros = zero_page();
  A3VT_CHECK_ARG(zeros != nullptr);
  const StackLayout L = stack_layout(batch, n_vert, in_features, hidden, num_layers, cut_len, 1, gemm_bf16);
  const StackStash S = stack_stash(batch, n_vert, hidden, num_layers, cut_len, gemm_bf16);
  const size_t m = (size_t)batch * n_vert;
  const int cpad = pad4(cut_len);
  const int last = num_layers - 1;

  const SplitRef sref = split_ref(split);
  int32_t *heavyT;
  if (int rc = hub_rows(rowptrT, n_vert, max_degreeT, scratch + L.heavy, &heavyT, s)) return rc;
  // the layout the forward left in this stash (recorded by a3vt_gcn_stack_fwd); a stash this library did not write: by shape
  const StackPlan P = stack_plan(gemm_bf16, batch, n_vert, hidden, num_layers, cut_len, max_degreeT, split,
                                 masks ? stash_layout_lookup(masks) : 0);
  const bool quad = P.quad;
  const int qcols = P.qcols, rm_ld = P.rm_ld;
  const size_t rm_off = P.rm_off;
  int32_t *ellT = reinterpret_cast<int32_t *>(scratch + L.ell);
  if (int rc = launch_stack_ell(P, split, rowptrT, colT, valT, n_vert, ellT, s)) return rc;
  // ---- output layer
  {
    const float *xl = num_layers == 1 ? feats : acts + S.act(last - 1);
    const float *x = xl + rm_off - qcols;                 // hybrid rows: see a3vt_gcn_stack_fwd (qcols = 0: plain rows)
    const int ldx = num_layers == 1 ? ld_feats : rm_ld;
    const int k = num_layers == 1 ? in_features : hidden;
    float *gprev = num_layers == 1 ? grad_feats : scratch + L.ping[0];
    const int ldg = num_layers == 1 ? ld_feats : hidden;
    ProfScope pso(PROF_OUT, s);
    if (int rc = launch_thin_bwd(x, ldx, k, weights[last], rowptrT, colT, valT, heavyT, n_vert, batch, grad_update,
                                 scratch + L.z3, num_layers > 1, gprev, ldg, ldg, scratch + L.thin_dw_slab,
                                 scratch + L.thin_db_slab, quad ? scratch + L.gq : nullptr, cpad / 4, quad ? xl : nullptr,
                                 qcols / 4, s, split ? &sref : nullptr))
      return rc;
    if (int rc = reduce_output_grads(scratch + L.thin_dw_slab, scratch + L.thin_db_slab, k, grad_weights[last], grad_biases[last],
                                     acc, s))
      return rc;
  }

  // zero-padded weight images (Bt = W_i for dX) of the hidden layers; mode 3: layers 1 .. L-2 as three bf16 images each
  // (layer 0's dX has the plain epilogue: exact kernels, fp32 image)
  if (P.x3)
    if (int rc = launch_stack_images(GEMM_FP32X3, 0, weights, 1, last, in_features, hidden, ld_feats, hidden, scratch + L.wt,
                                     L.wt_stride, s))
      return rc;
  if (int rc = launch_stack_images(GEMM_FP32, 0, weights, 0, P.x3 ? 1 : last, in_features, hidden, ld_feats, hidden,
                                   scratch + L.wt, L.wt_stride, s))
    return rc;

  // ---- hidden layers, last to first.  g = dL/dY_i already multiplied by the ReLU mask of layer i.
  const int db_rows = quad ? batch : csr_bwd_num_slabs(batch, n_vert);   // partial rows per layer (L.db_layer_stride holds either)
  int cur = 0;
  for (int i = last - 1; i >= 0; --i) {
    float *g = scratch + L.ping[cur];
    float *dza = scratch + L.za;
    const float *xl = i == 0 ? feats : acts + S.act(i - 1);
    const bool xhyb = quad && i > 0;                  // X_i = output of layer i-1: hybrid rows on the channel-sliced path
    const float *x = xhyb ? xl + rm_off - qcols : xl;
    const int ldx = i == 0 ? ld_feats : (xhyb ? rm_ld : hidden);
    const int kin = i == 0 ? in_features : hidden;

    // bias gradient + A^T gather on the aggregated channels
    if (cut_len > 0 && quad) {
      const uint8_t *sq = masks + S.signq(i);
      ProfScope psa(PROF_AGG, s);
      // the (mesh, channel) partials of this layer: summed over the meshes by ONE launch for all layers behind the loop
      if (P.qsplit) {
        if (int rc = launch_csrqs_bwd(scratch + L.gq, cut_len, ellT, n_vert, batch, dza, sq,
                                      scratch + L.db_slab + (size_t)i * L.db_layer_stride, s))
          return rc;
      } else if (int rc = launch_csrq_bwd(scratch + L.gq, cut_len, rowptrT, colT, valT, heavyT, ellT, n_vert, batch, dza, sq,
                                          scratch + L.db_slab + (size_t)i * L.db_layer_stride, s)) {
        return rc;
      }
    } else if (cut_len > 0) {
      ProfScope psa(PROF_AGG, s);
      if (int rc = launch_csr_bwd(g, hidden, cut_len, rowptrT, colT, valT, heavyT, n_vert, batch, dza, L.ldza,
                                  scratch + L.db_slab + (size_t)i * L.db_layer_stride, s))
        return rc;
      // (channels >= cut_len are dead bias parameters (model.py:358): written as exact zeros by the reduce behind the loop)
    } else if (!acc) {
      if (int rc = launch_fill_zero(grad_biases[i], hidden, s)) return rc;
    }

    // dW_i = X_i^T dZ
    DwArgs d{};
    if (xhyb) {   // staged image [16][hidden], sources: quad-major + row-major parts
      d.ldx_src = rm_ld;
      d.xq = xl;
      d.xq_nvert = n_vert;
      d.xq_quads = qcols / 4;
    }
    if (quad) {
      d.z0q_nvert = n_vert;
      d.z0q_quads = cpad / 4;
    }
    d.z0 = dza;
    d.ldz0 = L.ldza;
    d.z1 = g;
    d.ldz1 = hidden;
    d.zsplit = cpad;
    d.zeros = zeros;
    d.slab = scratch + L.dw_slab;
    d.m = (int)m;
    d.n_out = hidden;
    d.mode = P.omode;
    const int ldxw = xhyb ? hidden : ldx;   // width of the rows the kernel stages
    if (P.x3 && i > 0) {   // hidden layer of a mode-3 stack: the split-operand kernel when it takes the shape (one pass of kin columns)
      d.mode = GEMM_FP32X3;
      d.x = x;
      d.ldx = ldxw;
      d.k_in = kin;
      if (!dw3_ok(d)) d.mode = P.omode;
    }
    if (int rc = dw_panels(d, x, ldxw, kin, scratch + L.panel, grad_weights[i], acc, true, s)) return rc;

    // dX_i = dZ W_i^T  (masked by the ReLU of layer i-1, whose output is X_i)
    RowGemmArgs r{};
    r.a0 = dza;
    r.lda0 = L.ldza;
    if (quad) {   // dZa is quad-major (csrq_kernel<1>)
      r.a0q_nvert = n_vert;
      r.a0q_quads = cpad / 4;
    }
    r.a1 = g;
    r.lda1 = hidden;
    r.ksplit = cpad;
    r.bt = scratch + L.wt + L.wt_stride * i;
    r.ldb = pad16(hidden);
    r.zeros = zeros;
    r.m = (int)m;
    r.k = hidden;
    r.n_store = i == 0 ? ld_feats : hidden;
    r.mode = P.x3 && i > 0 ? GEMM_FP32X3 : P.omode;
    if (i == 0) {
      r.c = grad_feats;
      r.ldc = ld_feats;
      if (int rc = launch_rowgemm(r, EPI_PLAIN, s)) return rc;
    } else {
      r.c = scratch + L.ping[cur ^ 1];
      r.ldc = hidden;
      // X_i is the output of layer i-1: its ReLU signs were saved by that layer's forward launches
      r.maskb = const_cast<uint8_t *>(masks) + S.signs(i - 1);
      r.mld = S.mld;
      r.moff = cpad / 4;
      r.csplit = cut_len;
      if (quad) {   // gradient columns [0, cpad) go quad-major (unmasked below cut_len) to the next aggregation
        r.c2 = scratch + L.gq;
        r.zq_nvert = n_vert;
        r.zq_quads = cpad / 4;
        r.trash = scratch + L.z3;
      }
      {
        ProfScope ps(PROF_GEMM_DX, s);
        if (int rc = launch_rowgemm(r, EPI_DX_MASK, s)) return rc;
      }
      cur ^= 1;
    }
  }
  // bias gradients of all hidden layers from their partial rows (one per mesh on the channel-sliced path, one per row-walk
  // workgroup otherwise): one launch instead of one per layer (19 x 3.8-5.5 us per stack call)
  if (cut_len > 0)
    if (int rc = reduce_bias_partials(scratch + L.db_slab, L.db_layer_stride, db_rows, cpad, cut_len, hidden, last, grad_biases, acc, s))
      return rc;
  return 0;
}

// ---- one layer on its own (GCN_layer.forward for the auto-encoder / DDQN layer loops)
namespace {
struct LayerLayout {
  size_t wt, za, ga, dz, panel, dw_slab, db_slab, heavy, total;
  int ldza;   // row stride of za: cpad, or 4 (dummy rows) without aggregated channels
};
LayerLayout layer_layout(int batch, int n_vert, int ld_x, int n_out, int cut_len, int need_backward) {
  LayerLayout L{};
  const size_t m = (size_t)batch * n_vert;
  const int cpad = pad4(cut_len), npad = pad4(n_out);
  L.ldza = cpad > 4 ? cpad : 4;
  Arena a;
  const size_t wt_fwd = (size_t)rowgemm_bt_rows(n_out) * pad16(ld_x);
  const size_t wt_bwd = (size_t)rowgemm_bt_rows(ld_x) * pad16(npad);
  L.wt = a.take(wt_fwd > wt_bwd ? wt_fwd : wt_bwd);
  L.za = a.take(m * L.ldza);  // forward: raw Z of the aggregated channels; backward: 4-float dummy rows
  L.heavy = a.take(csr_heavy_scratch_ints(n_vert));
  if (need_backward) {
    L.ga = a.take(m * L.ldza);
    L.dz = a.take(m * npad);
    L.panel = a.take(ld_x > 304 ? m * 300 : 0);
    const int kin = ld_x > 304 ? 300 : ld_x;
    L.dw_slab = a.take((size_t)dw_num_slabs(n_out) * kin * n_out);
    L.db_slab = a.take((size_t)csr_bwd_num_slabs(batch, n_vert) * L.ldza);
  }
  L.total = a.off;
  return L;
}
int check_layer_dims(int ld_x, int in_features, int n_out, int cut_len) {
  if (ld_x % 4 != 0 || ld_x < in_features || ld_x > 600 || in_features < 1) {
    set_error("gcn_layer: ld_x=%d must be a multiple of 4, >= in_features=%d and <= 600", ld_x, in_features);
    return -1;
  }
  if (n_out < 1 || n_out > 304 || cut_len < 0 || cut_len > n_out) {
    set_error("gcn_layer: out_features=%d (1..304) cut_len=%d unsupported", n_out, cut_len);
    return -1;
  }
  if (in_features > 304 && in_features % 4 != 0) {
    set_error("gcn_layer: in_features=%d > 304 must be a multiple of 4", in_features);
    return -1;
  }
  return 0;
}
// What a3vt_gcn_layer_* and a3vt_qnet_input_* share: a single layer behind its product, and its backward up to dZ.
// Forward: y[:, :c] = act(A za[:, :c] + bias) on the aggregated channels (heavy_slot: the layout's hub-row region)
int layer_fwd_tail(const float *za, int ldza, const float *bias, int cut_len, int relu, const int32_t *rowptr, const int32_t *col,
                   const float *val, int max_degree, int n_vert, int batch, float *y, int ld_y, float *heavy_slot, hipStream_t s) {
  if (cut_len <= 0) return 0;
  int32_t *heavy;
  if (int rc = hub_rows(rowptr, n_vert, max_degree, heavy_slot, &heavy, s)) return rc;
  return launch_csr_fwd(za, ldza, bias, cut_len, rowptr, col, val, heavy, n_vert, batch, y, ld_y, nullptr, 0, relu, s);
}
// Backward: the gradient through the activation, aggregated columns to `ga`, the rest straight into the merged dZ rows `dz`
// [M][pad4(n_out)]; then dZ[:, :c] = A^T G[:, :c] (columns c..cpad pass through), bias gradient = column sums of G[:, :c]
int layer_bwd_tail(const float *grad_y, int ld_gy, const float *y, int ld_y, int relu, int n_out, int cut_len,
                   const int32_t *rowptrT, const int32_t *colT, const float *valT, int max_degreeT, int n_vert, int batch, float *ga,
                   float *dz, float *db_slab, float *heavy_slot, float *grad_bias, hipStream_t s) {
  const int cpad = pad4(cut_len), npad = pad4(n_out);
  if (int rc = launch_relu_split(grad_y, ld_gy, y, ld_y, relu, n_out, cpad, npad, (long long)batch * n_vert, ga, dz, s)) return rc;
  if (int rc = launch_fill_zero(grad_bias, n_out, s)) return rc;
  if (cut_len <= 0) return 0;
  int32_t *heavyT;
  if (int rc = hub_rows(rowptrT, n_vert, max_degreeT, heavy_slot, &heavyT, s)) return rc;
  if (int rc = launch_csr_bwd(ga, cpad, cut_len, rowptrT, colT, valT, heavyT, n_vert, batch, dz, npad, db_slab, s)) return rc;
  return launch_slab_reduce(db_slab, csr_bwd_num_slabs(batch, n_vert), cpad, cut_len, grad_bias, s);
}
}  // namespace

size_t a3vt_gcn_layer_scratch_bytes(int batch, int n_vert, int ld_x, int out_features, int cut_len, int need_backward) {
  return layer_layout(batch, n_vert, ld_x, out_features, cut_len, need_backward).total * sizeof(float);
}

int a3vt_gcn_layer_fwd(const float *x, int ld_x, int in_features, const float *weight, const float *bias,
                       int out_features, int cut_len, int relu, const int32_t *rowptr, const int32_t *col,
                       const float *val, int max_degree, int n_vert, int batch, int gemm_bf16, float *y, int ld_y,
                       float *scratch, void *stream) {
  A3VT_CHECK_ARG(x && weight && bias && rowptr && col && val && y && scratch && n_vert > 0 && batch > 0);
  if (int rc = check_layer_dims(ld_x, in_features, out_features, cut_len)) return rc;
  A3VT_CHECK_ARG(ld_y % 4 == 0 && ld_y >= out_features);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float *zeros = zero_page();
  A3VT_CHECK_ARG(zeros != nullptr);
  const LayerLayout L = layer_layout(batch, n_vert, ld_x, out_features, cut_len, 0);
  const size_t m = (size_t)batch * n_vert;
  float *wt = scratch + L.wt;
  if (int rc = launch_transpose_pad(weight, in_features, out_features, wt, rowgemm_bt_rows(out_features), pad16(ld_x), s))
    return rc;
  RowGemmArgs g{};
  g.a0 = g.a1 = x;
  g.lda0 = g.lda1 = ld_x;
  g.ksplit = ld_x;
  g.bt = wt;
  g.ldb = pad16(ld_x);
  g.zeros = zeros;
  g.m = (int)m;
  g.k = ld_x;
  g.n_store = out_features;
  g.c = y;
  g.ldc = ld_y;
  g.c2 = scratch + L.za;
  g.ldc2 = L.ldza;
  g.csplit = cut_len;
  g.no_relu = relu ? 0 : 1;
  g.mode = gemm_bf16 == GEMM_BF16_OPERANDS ? GEMM_BF16_OPERANDS : GEMM_FP32;   // (mode 3 is a stack mode: a lone layer runs exact)
  if (int rc = launch_rowgemm(g, EPI_FWD_HIDDEN, s)) return rc;
  return layer_fwd_tail(scratch + L.za, L.ldza, bias, cut_len, relu ? 1 : 0, rowptr, col, val, max_degree, n_vert, batch, y, ld_y,
                        scratch + L.heavy, s);
}

int a3vt_gcn_layer_bwd(const float *x, int ld_x, int in_features, const float *weight, int out_features, int cut_len,
                       int relu, const int32_t *rowptrT, const int32_t *colT, const float *valT, int max_degreeT,
                       int n_vert, int batch, int gemm_bf16, const float *y, int ld_y, const float *grad_y, int ld_gy,
                       float *grad_weight, float *grad_bias, float *grad_x, float *scratch, void *stream) {
  A3VT_CHECK_ARG(x && weight && rowptrT && colT && valT && grad_y && grad_weight && grad_bias && grad_x && scratch);
  A3VT_CHECK_ARG(n_vert > 0 && batch > 0 && ld_gy >= out_features && (!relu || (y && ld_y >= out_features)));
  if (int rc = check_layer_dims(ld_x, in_features, out_features, cut_len)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float *zeros = zero_page();
  A3VT_CHECK_ARG(zeros != nullptr);
  const LayerLayout L = layer_layout(batch, n_vert, ld_x, out_features, cut_len, 1);
  const size_t m = (size_t)batch * n_vert;
  const int npad = pad4(out_features);
  float *dz = scratch + L.dz;
  if (int rc = layer_bwd_tail(grad_y, ld_gy, y, ld_y, relu ? 1 : 0, out_features, cut_len, rowptrT, colT, valT, max_degreeT, n_vert,
                              batch, scratch + L.ga, dz, scratch + L.db_slab, scratch + L.heavy, grad_bias, s))
    return rc;
  // dW = X^T dZ
  DwArgs d{};
  d.z0 = scratch + L.za;  // zsplit = 0: never consumed, only staged
  d.ldz0 = 4;
  d.z1 = dz;
  d.ldz1 = npad;
  d.zsplit = 0;
  d.zeros = zeros;
  d.slab = scratch + L.dw_slab;
  d.m = (int)m;
  d.n_out = out_features;
  d.mode = gemm_bf16 == GEMM_BF16_OPERANDS ? GEMM_BF16_OPERANDS : GEMM_FP32;
  if (int rc = dw_panels(d, x, ld_x, in_features, scratch + L.panel, grad_weight, 0, false, s)) return rc;
  // dX = dZ W^T
  float *wp = scratch + L.wt;
  if (int rc = launch_copy_pad(weight, in_features, out_features, wp, rowgemm_bt_rows(ld_x), pad16(npad), s)) return rc;
  RowGemmArgs r{};
  r.a0 = scratch + L.za;
  r.lda0 = 4;
  r.ksplit = 0;
  r.a1 = dz;
  r.lda1 = npad;
  r.bt = wp;
  r.ldb = pad16(npad);
  r.zeros = zeros;
  r.m = (int)m;
  r.k = npad;
  r.n_store = ld_x;
  r.mode = gemm_bf16 == GEMM_BF16_OPERANDS ? GEMM_BF16_OPERANDS : GEMM_FP32;
  r.c = grad_x;
  r.ldc = ld_x;
  return launch_rowgemm(r, EPI_PLAIN, s);
}

// ---- the DDQN learner: TD target + loss (ddqn.hip), the graph model's fused input layer (qnet_input.hip) ------------------------
int a3vt_ddqn_td(const float *q_cur, const float *q_next_online, const float *q_next_target, const float *mask, const float *actions,
                 const float *rewards, const float *denom, int batch, int num_actions, int budget, float gamma, float *loss,
                 float *diff, int32_t *best_next, float *target, void *stream) {
  A3VT_CHECK_ARG(batch >= 1 && batch <= kTdMaxBatch && num_actions >= 1 && num_actions <= kTdMaxActions);
  A3VT_CHECK_ARG(q_cur && q_next_online && q_next_target && mask && actions && rewards);
  A3VT_CHECK_ARG(loss && diff && best_next && target);
  return launch_ddqn_td(q_cur, q_next_online, q_next_target, mask, actions, rewards, denom, batch, num_actions, budget, gamma, loss,
                        diff, best_next, target, static_cast<hipStream_t>(stream));
}

int a3vt_ddqn_td_bwd(const float *diff, const float *actions, const float *grad_loss, int batch, int num_actions, float *dq_cur,
                     void *stream) {
  A3VT_CHECK_ARG(batch >= 1 && batch <= kTdMaxBatch && num_actions >= 1 && num_actions <= kTdMaxActions);
  A3VT_CHECK_ARG(diff && actions && grad_loss && dq_cur);
  return launch_ddqn_td_bwd(diff, actions, grad_loss, batch, num_actions, dq_cur, static_cast<hipStream_t>(stream));
}

// ---- the nearest-neighbour policy's bank lookup (latent_nn.hip) -----------------------------------------------------------------
namespace {
bool latent_dims_ok(int n_queries, int bank_rows, int k) {
  return n_queries >= 1 && n_queries <= kLatentMaxQueries && bank_rows >= 1 && bank_rows <= kLatentMaxRows && k >= 1 && k <= kLatentMaxK;
}
}  // namespace

size_t a3vt_latent_nearest_scratch_bytes(int n_queries, int bank_rows, int k) {
  if (!latent_dims_ok(n_queries, bank_rows, k)) return 0;
  return (size_t)n_queries * bank_rows * sizeof(float);
}

int a3vt_latent_nn_tile(void) { return kLatentTile; }
int a3vt_latent_nn_query_floats(void) { return kLatentQueryFloats; }
int a3vt_latent_nn_cached_rows(void) { return kLatentCachedRows; }

int a3vt_latent_nearest(const float *bank, const int32_t *bank_actions, int bank_rows, int dim, const float *queries, const float *taken,
                        int n_queries, int num_actions, int k, int32_t *idx, float *dist, int32_t *action, int32_t *rank, void *scratch,
                        void *stream) {
  if (!latent_dims_ok(n_queries, bank_rows, k) || dim < 1 || dim > kLatentMaxDim || num_actions < 1 || num_actions > kTdMaxActions) {
    set_error("latent_nearest: bank_rows=%d (1..%d) dim=%d (1..%d) n_queries=%d (1..%d) num_actions=%d (1..%d) k=%d (1..%d) unsupported",
              bank_rows, kLatentMaxRows, dim, kLatentMaxDim, n_queries, kLatentMaxQueries, num_actions, kTdMaxActions, k, kLatentMaxK);
    return -1;
  }
  A3VT_CHECK_ARG(bank && queries && idx && dist && scratch);
  A3VT_CHECK_ARG((bank_actions && action && rank) || (!bank_actions && !action && !rank));
  const unsigned row_align = dim % 4 == 0 ? 16 : 4;   // (16-byte loads along dim when every row starts on one)
  A3VT_CHECK_ARG(aligned_to(bank, row_align) && aligned_to(queries, row_align));
  A3VT_CHECK_ARG(aligned_to(bank_actions, 4) && aligned_to(taken, 4) && aligned_to(idx, 4) && aligned_to(dist, 4) && aligned_to(action, 4) &&
                 aligned_to(rank, 4) && aligned_to(scratch, 4));
  return launch_latent_nearest(bank, bank_actions, bank_rows, dim, queries, taken, n_queries, num_actions, k, idx, dist, action, rank,
                               scratch, static_cast<hipStream_t>(stream));
}

// ---- the dataset-specific policies' candidate tally (candidate_tally.hip) --------------------------------------------------------
int a3vt_candidate_tally(const float *scores, const int32_t *candidates, const float *first_score, const float *taken, int K, int E, int A,
                         double unvisited, double *sums, double *checks, double *votes, int32_t *best, float *best_score, void *stream) {
  if (K < 1 || K > kTallyMaxCandidates || E < 1 || E > kTallyMaxElements || A < 1 || A > kTallyMaxActions) {
    set_error("candidate_tally: K=%d (1..%d) E=%d (1..%d) A=%d (1..%d) unsupported", K, kTallyMaxCandidates, E, kTallyMaxElements, A,
              kTallyMaxActions);
    return -1;
  }
  if (check_ptrs("candidate_tally", {{"scores", scores, true, 4, "required"},
                                     {"candidates", candidates, true, 4, "required"},
                                     {"first_score", first_score, sums != nullptr, 4, "required with sums"},
                                     {"taken", taken, false, 4, ""},
                                     {"sums", sums, checks != nullptr, 8, "sums and checks go together"},
                                     {"checks", checks, sums != nullptr, 8, "sums and checks go together"},
                                     {"votes", votes, false, 8, ""},
                                     {"best", best, votes != nullptr, 4, "required with votes"},
                                     {"best_score", best_score, false, 4, ""}}))
    return -1;
  return launch_candidate_tally(scores, candidates, first_score, taken, K, E, A, unvisited, sums, checks, votes, best, best_score,
                                static_cast<hipStream_t>(stream));
}

// ---- the candidate inputs of a greedy step from the per-episode touch table (touch_assemble.hip) ---------------------------------
namespace {
LaunchCounts<1> g_touch_assemble_launches;
}  // namespace

int a3vt_touch_assemble(const float *table_charts, const int32_t *table_codes, const float *state_charts, const float *state_masks,
                        const int32_t *candidates, int K, int E, int A, int F, int G, int C, int slot, float *charts, float *masks,
                        void *stream) {
  const char *who = "touch_assemble";
  if (check_range(who, "K", K, 1, INT_MAX) || check_range(who, "E", E, 1, INT_MAX) || check_range(who, "A", A, 1, INT_MAX) ||
      check_range(who, "F", F, 1, INT_MAX) || check_range(who, "G", G, 1, INT_MAX) || check_range(who, "C", C, 1, INT_MAX) ||
      check_range(who, "slot", slot, 0, G - 1))
    return -1;
  const double floats = 3.0 * K * E * F * G * C;   // (six factors below 2^31 each: exact in a double wherever it decides)
  if (floats >= 2147483648.0) {
    set_error("%s: K*E*F*G*C*3=%.0f (K=%d E=%d F=%d G=%d C=%d) is not below 2147483648", who, floats, K, E, F, G, C);
    return -1;
  }
  if (check_ptrs(who, {{"table_charts", table_charts, true, 4, "required"},
                       {"table_codes", table_codes, true, 4, "required"},
                       {"state_charts", state_charts, true, 4, "required"},
                       {"state_masks", state_masks, true, 4, "required"},
                       {"candidates", candidates, true, 4, "required"},
                       {"charts", charts, true, 4, "required"},
                       {"masks", masks, true, 4, "required"}}))
    return -1;
  if (int rc = launch_touch_assemble(table_charts, table_codes, state_charts, state_masks, candidates, K, E, A, F, G, C, slot, charts, masks,
                                     static_cast<hipStream_t>(stream)))
    return rc;
  g_touch_assemble_launches.add(0, 1);
  return 0;
}

int a3vt_touch_assemble_launches(long long *counts, int reset) { return g_touch_assemble_launches.read(counts, reset); }

// ---- the touch chart predictor's head: fc, template, finger frame and slot rule (chart_head.hip) ---------------------------------
namespace {
LaunchCounts<1> g_chart_head_launches;
}  // namespace

int a3vt_touch_chart_head(const float *features, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                          const float *b3, const float *tmpl, const float *rot, const float *pos, const int32_t *code, int n, float *rows,
                          float *charts, float *masks, void *stream) {
  const char *who = "touch_chart_head";
  if (check_range(who, "n", n, 1, INT_MAX)) return -1;
  const double floats = (double)kHeadIn * n;
  if (floats >= 2147483648.0) {
    set_error("%s: n*%d=%.0f (n=%d) is not below 2147483648", who, kHeadIn, floats, n);
    return -1;
  }
  if (check_ptrs(who, {{"features", features, true, 16, "required"},
                       {"w1", w1, true, 16, "required"},
                       {"b1", b1, true, 4, "required"},
                       {"w2", w2, true, 16, "required"},
                       {"b2", b2, true, 4, "required"},
                       {"w3", w3, true, 16, "required"},
                       {"b3", b3, true, 4, "required"},
                       {"tmpl", tmpl, true, 4, "required"},
                       {"rot", rot, true, 4, "required"},
                       {"pos", pos, true, 4, "required"},
                       {"code", code, true, 4, "required"},
                       {"rows", rows, true, 16, "required"},
                       {"charts", charts, masks != nullptr, 4, "charts and masks go together"},
                       {"masks", masks, charts != nullptr, 4, "charts and masks go together"}}))
    return -1;
  if (int rc = launch_touch_chart_head(features, w1, b1, w2, b2, w3, b3, tmpl, rot, pos, code, n, rows, charts, masks,
                                       static_cast<hipStream_t>(stream)))
    return rc;
  g_chart_head_launches.add(0, 1);
  return 0;
}

int a3vt_touch_chart_head_launches(long long *counts, int reset) { return g_chart_head_launches.read(counts, reset); }

// ---- the rendered touch sampler (touch_render.hip) ---------------------------------------------------------------------------------
namespace {
// The finish launch's own arguments (shared by both entries): 0, or -1 with the message set.
int touch_finish_check(const char *who, const float *cam_pos, const float *cam_rot, int I, float max_depth, float yfov, const float *depth,
                       const float *touch, const float *points, const int32_t *count, const int32_t *status) {
  if (check_range(who, "I", I, 1, kTouchMaxImages)) return -1;
  if (!(max_depth > 0.f)) {
    set_error("%s: max_depth=%g must be > 0", who, (double)max_depth);
    return -1;
  }
  if (!(yfov > 0.f && (double)yfov < 3.14159265358979323846)) {
    set_error("%s: yfov=%g outside (0, pi)", who, (double)yfov);
    return -1;
  }
  return check_ptrs(who, {{"cam_pos", cam_pos, true, 4, "required"},
                          {"cam_rot", cam_rot, true, 4, "required"},
                          {"depth", depth, true, 4, "required"},
                          {"touch", touch, false, 4, ""},
                          {"points", points, count != nullptr, 4, "points and count go together"},
                          {"count", count, points != nullptr, 4, "points and count go together"},
                          {"status", status, true, 4, "required"}});
}
}  // namespace

int a3vt_touch_finish(const float *depth, const float *cam_pos, const float *cam_rot, int I, float max_depth, float yfov, float *touch,
                      float *points, int32_t *count, int32_t *status, void *stream) {
  if (touch_finish_check("touch_finish", cam_pos, cam_rot, I, max_depth, yfov, depth, touch, points, count, status)) return -1;
  return launch_touch_finish(depth, cam_pos, cam_rot, I, max_depth, yfov, touch, points, count, status, static_cast<hipStream_t>(stream));
}

int a3vt_touch_render(const float *verts, int V, const int32_t *faces, int F, const int32_t *face_offset, int M, const int32_t *image_mesh,
                      const float *cam_pos, const float *cam_rot, int I, float max_depth, float yfov, float znear, float zfar, float *depth,
                      float *touch, float *points, int32_t *count, int32_t *status, void *stream) {
  if (check_range("touch_render", "M", M, 1, kTouchMaxMeshes)) return -1;
  if (V < 0 || V > kTouchMaxIndex || F < 0 || F > kTouchMaxIndex) {
    set_error("touch_render: V=%d F=%d outside 0..%d", V, F, kTouchMaxIndex);
    return -1;
  }
  if (!(znear > 0.f)) {
    set_error("touch_render: znear=%g must be > 0", (double)znear);
    return -1;
  }
  if (!(znear < zfar)) {
    set_error("touch_render: zfar=%g must be above znear=%g", (double)zfar, (double)znear);
    return -1;
  }
  if (check_ptrs("touch_render", {{"verts", verts, V > 0, 4, "required when V > 0"},
                                  {"faces", faces, F > 0, 4, "required when F > 0"},
                                  {"face_offset", face_offset, true, 4, "required"},
                                  {"image_mesh", image_mesh, true, 4, "required"}}))
    return -1;
  if (touch_finish_check("touch_render", cam_pos, cam_rot, I, max_depth, yfov, depth, touch, points, count, status)) return -1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = launch_touch_depth(verts, V, faces, F, face_offset, M, image_mesh, cam_pos, cam_rot, I, yfov, znear, zfar, depth, s)) return rc;
  return launch_touch_finish(depth, cam_pos, cam_rot, I, max_depth, yfov, touch, points, count, status, s);
}

// ---- the renderer's outputs as a data set stores them (touch_pack.hip) -------------------------------------------------------------
namespace {
LaunchCounts<1> g_touch_pack_launches;
}  // namespace

int a3vt_touch_pack(const float *touch, const float *points, const int32_t *count, const int32_t *status, int I, int capacity,
                    uint8_t *touch_u8, int32_t *offsets, float *cloud, void *stream) {
  const char *who = "touch_pack";
  if (check_range(who, "I", I, 1, kTouchMaxImages) || check_range(who, "capacity", capacity, 0, INT_MAX)) return -1;
  const bool cloudy = points || count || status || offsets || cloud;
  if (!touch && !touch_u8 && !cloudy) {
    set_error("%s: touch=NULL and points=NULL: nothing to pack", who);
    return -1;
  }
  if (check_ptrs(who, {{"touch", touch, touch_u8 != nullptr, 16, "touch and touch_u8 go together"},
                       {"touch_u8", touch_u8, touch != nullptr, 4, "touch and touch_u8 go together"},
                       {"points", points, cloudy, 4, "points, count, status and offsets go together"},
                       {"count", count, cloudy, 4, "points, count, status and offsets go together"},
                       {"status", status, cloudy, 4, "points, count, status and offsets go together"},
                       {"offsets", offsets, cloudy, 4, "points, count, status and offsets go together"},
                       {"cloud", cloud, cloudy && capacity > 0, 4, "required with points when capacity > 0"}}))
    return -1;
  if (int rc = launch_touch_pack(touch, points, count, status, I, capacity, touch_u8, offsets, cloud, static_cast<hipStream_t>(stream)))
    return rc;
  g_touch_pack_launches.add(0, 1);
  return 0;
}

int a3vt_touch_pack_launches(long long *counts, int reset) { return g_touch_pack_launches.read(counts, reset); }

// ---- the finger closing of the kinematic grasp (grasp_close.hip) -------------------------------------------------------------------
namespace {
LaunchCounts<2> g_grasp_launches;

// The HOST hand table (28 x 26 doubles) and rest angles as the kernel's argument block: 0, or -1 with the message set.
int grasp_hand(const char *who, const double *table, const double *q0, int steps, GraspHand *hand) {
  auto finite = [](double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; };
  for (int row = 0; row < kGraspLinks; ++row) {
    const double *t = table + row * kGraspTableCols;
    for (int col = 0; col < kGraspTableCols; ++col) {
      if (!finite(t[col])) {
        set_error("%s: hand_table[%d][%d]=%g is not finite", who, row, col, t[col]);
        return -1;
      }
    }
    const int c = row / kGraspChain, k = row % kGraspChain;
    const int parent = (int)t[0], want_parent_lo = k == 0 ? -1 : c * kGraspChain, want_parent_hi = k == 0 ? -1 : row - 1;
    if ((double)parent != t[0] || parent < want_parent_lo || parent > want_parent_hi) {
      set_error("%s: hand_table[%d][0]=%g: the parent of link %d of chain %d must lie in %d..%d", who, row, t[0], k, c, want_parent_lo,
                want_parent_hi);
      return -1;
    }
    const double want_type = k < kGraspJoints ? 1.0 : 0.0;
    if (t[1] != want_type) {
      set_error("%s: hand_table[%d][1]=%g: link %d of a chain must be %s", who, row, t[1], k, k < kGraspJoints ? "revolute (1)" : "fixed (0)");
      return -1;
    }
    const double axis2 = t[14] * t[14] + t[15] * t[15] + t[16] * t[16];
    if (t[1] != 0.0 && !(axis2 > 0.999 && axis2 < 1.001)) {
      set_error("%s: hand_table[%d][14..16]: the axis has squared length %g, not 1", who, row, axis2);
      return -1;
    }
    if (t[17] > t[18]) {
      set_error("%s: hand_table[%d][17]=%g (lower) is above [18]=%g (upper)", who, row, t[17], t[18]);
      return -1;
    }
    if ((t[19] != 0.0 && t[19] != 1.0) || t[23] < 0.0 || t[24] < 0.0 || t[25] < 0.0) {
      set_error("%s: hand_table[%d][19]=%g must be 0 or 1 and the half-extents [23..25] must not be negative", who, row, t[19]);
      return -1;
    }
    if (q0 && !finite(q0[row])) {
      set_error("%s: q0[%d]=%g is not finite", who, row, q0[row]);
      return -1;
    }
    GraspLink &L = hand->link[row];
    for (int i = 0; i < 3; ++i) L.xyz[i] = (float)t[2 + i], L.axis[i] = (float)t[14 + i], L.bc[i] = (float)t[20 + i], L.bh[i] = (float)t[23 + i];
    for (int i = 0; i < 9; ++i) L.rot[i] = (float)t[5 + i];
    const double rest = q0 ? q0[row] : 0.0;
    L.q0 = (float)rest;
    L.upper = (float)t[18];
    L.delta = (float)((t[18] - rest) / (double)steps);
    L.parent = parent < 0 ? -1 : parent - c * kGraspChain;
    L.revolute = t[1] != 0.0;
    L.has_box = t[19] != 0.0;
  }
  // reach: a link's origin is no further from the chain's first joint than the joint offsets on its path sum to, and no point of
  // its box further from the origin than |centre| + |half|
  auto norm = [](const double *v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
  for (int c = 0; c < kGraspFingers; ++c) {
    double path[kGraspChain] = {0.0}, reach = 0.0;
    for (int k = 0; k < kGraspChain; ++k) {
      const double *t = table + (c * kGraspChain + k) * kGraspTableCols;
      if (k > 0) path[k] = path[(int)t[0] - c * kGraspChain] + norm(t + 2);
      if (t[19] != 0.0) reach = fmax(reach, path[k] + norm(t + 20) + norm(t + 23));
    }
    hand->reach[c] = (float)(reach * (1.0 + 1e-6));
  }
  return 0;
}
}  // namespace

int a3vt_grasp_close(const float *verts, int V, const int32_t *faces, int F, const int32_t *face_offset, int M, const int32_t *grasp_mesh,
                     const float *base_pos, const float *base_rot, int G, const double *hand_table, const double *q0, int steps,
                     float *q_out, int32_t *blocked_step, float *link_pos, float *link_rot, float *frame_pos, float *frame_rot,
                     void *stream) {
  const char *who = "grasp_close";
  if (check_range(who, "G", G, 0, kGraspMaxGrasps) || check_range(who, "M", M, 1, kGraspMaxMeshes) ||
      check_range(who, "V", V, 0, kGraspMaxIndex) || check_range(who, "F", F, 0, kGraspMaxIndex) ||
      check_range(who, "steps", steps, 1, kGraspMaxSteps))
    return -1;
  if (check_ptrs(who, {{"verts", verts, V > 0, 4, "required when V > 0"},
                       {"faces", faces, F > 0, 4, "required when F > 0"},
                       {"face_offset", face_offset, true, 4, "required (a host table)"},
                       {"grasp_mesh", grasp_mesh, G > 0, 4, "required when G > 0 (a host table)"},
                       {"base_pos", base_pos, G > 0, 4, "required when G > 0"},
                       {"base_rot", base_rot, G > 0, 4, "required when G > 0"},
                       {"hand_table", hand_table, true, 8, "required (a host table)"},
                       {"q0", q0, true, 8, "required (a host table)"},
                       {"q_out", q_out, G > 0, 4, "required when G > 0"},
                       {"blocked_step", blocked_step, G > 0, 4, "required when G > 0"},
                       {"link_pos", link_pos, G > 0, 4, "required when G > 0"},
                       {"link_rot", link_rot, G > 0, 4, "required when G > 0"},
                       {"frame_pos", frame_pos, G > 0, 4, "required when G > 0"},
                       {"frame_rot", frame_rot, G > 0, 4, "required when G > 0"}}))
    return -1;
  // the host tables' contents
  if (face_offset[0] < 0) {
    set_error("%s: face_offset[0]=%d is below 0", who, (int)face_offset[0]);
    return -1;
  }
  for (int m = 0; m < M; ++m) {
    if (face_offset[m + 1] < face_offset[m]) {
      set_error("%s: face_offset[%d]=%d is below face_offset[%d]=%d: offsets must not decrease", who, m + 1, (int)face_offset[m + 1], m,
                (int)face_offset[m]);
      return -1;
    }
  }
  if (face_offset[M] > F) {
    set_error("%s: face_offset[%d]=%d runs past F=%d", who, M, (int)face_offset[M], F);
    return -1;
  }
  for (int g = 0; g < G; ++g) {
    if (grasp_mesh[g] < 0 || grasp_mesh[g] >= M) {
      set_error("%s: grasp_mesh[%d]=%d outside 0..%d", who, g, (int)grasp_mesh[g], M - 1);
      return -1;
    }
  }
  GraspHand hand;
  if (grasp_hand(who, hand_table, q0, steps, &hand)) return -1;
  if (G == 0) return 0;
  int32_t *range = static_cast<int32_t *>(malloc(sizeof(int32_t) * 2 * (size_t)G));
  if (!range) {
    set_error("%s: no host memory for the ranges of G=%d grasps", who, G);
    return -1;
  }
  for (int g = 0; g < G; ++g) {
    range[g] = face_offset[grasp_mesh[g]];
    range[G + g] = face_offset[grasp_mesh[g] + 1];
  }
  const int rc = launch_grasp_close(verts, V, faces, range, range + G, base_pos, base_rot, G, hand, steps, q_out, blocked_step, link_pos,
                                    link_rot, frame_pos, frame_rot, static_cast<hipStream_t>(stream));
  free(range);
  if (rc < 0) return rc;
  g_grasp_launches.add(0, 1);
  g_grasp_launches.add(1, rc);
  return 0;
}

int a3vt_grasp_limit(int which) { return which == 0 ? kGraspCapacity : which == 1 ? kGraspPerLaunch : which == 2 ? kGraspTableCols : 0; }

double a3vt_grasp_reach(const double *hand_table, int chain) {
  GraspHand hand;
  if (!hand_table || chain < 0 || chain >= kGraspFingers) {
    set_error("grasp_reach: hand_table=%p chain=%d: a table and a chain in 0..%d", (const void *)hand_table, chain, kGraspFingers - 1);
    return -1.0;
  }
  if (grasp_hand("grasp_reach", hand_table, nullptr, 1, &hand)) return -1.0;
  return (double)hand.reach[chain];
}

int a3vt_grasp_launches(long long *counts, int reset) { return g_grasp_launches.read(counts, reset); }

// ---- the hand's placement without a hull (hull_place.hip) --------------------------------------------------------------------------
namespace {
LaunchCounts<2> g_hull_launches;
}  // namespace

int a3vt_hull_place(const float *verts, int V, const int32_t *vert_offset, int M, const double *directions, int A, double hand_distance,
                    const double *tip_offset, int32_t *status, float *base_pos, float *base_rot, int32_t *simplex, double *t, void *stream) {
  const char *who = "hull_place";
  auto finite = [](double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; };
  if (check_range(who, "M", M, 1, kHullMaxMeshes) || check_range(who, "A", A, 1, kHullMaxActions) ||
      check_range(who, "M*A", (long long)M * A, 1, kHullMaxPairs) || check_range(who, "V", V, 0, kHullMaxVerts))
    return -1;
  if (check_ptrs(who, {{"verts", verts, V > 0, 4, "required when V > 0"},
                       {"vert_offset", vert_offset, true, 4, "required (a host table)"},
                       {"directions", directions, true, 8, "required (a host table)"},
                       {"tip_offset", tip_offset, true, 8, "required (a host table)"},
                       {"status", status, true, 4, "required"},
                       {"base_pos", base_pos, true, 4, "required"},
                       {"base_rot", base_rot, true, 4, "required"},
                       {"simplex", simplex, true, 4, "required"},
                       {"t", t, true, 8, "required"}}))
    return -1;
  // the host tables' contents
  if (vert_offset[0] < 0) {
    set_error("%s: vert_offset[0]=%d is below 0", who, (int)vert_offset[0]);
    return -1;
  }
  for (int m = 0; m < M; ++m) {
    if (vert_offset[m + 1] < vert_offset[m]) {
      set_error("%s: vert_offset[%d]=%d is below vert_offset[%d]=%d: offsets must not decrease", who, m + 1, (int)vert_offset[m + 1], m,
                (int)vert_offset[m]);
      return -1;
    }
  }
  if (vert_offset[M] > V) {
    set_error("%s: vert_offset[%d]=%d runs past V=%d", who, M, (int)vert_offset[M], V);
    return -1;
  }
  for (int a = 0; a < A; ++a) {
    const double *d = directions + 3 * a;
    for (int i = 0; i < 3; ++i) {
      if (!finite(d[i])) {
        set_error("%s: directions[%d][%d]=%g is not finite", who, a, i, d[i]);
        return -1;
      }
    }
    if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) {
      set_error("%s: directions[%d] is zero", who, a);
      return -1;
    }
  }
  if (!finite(hand_distance)) {
    set_error("%s: hand_distance=%g is not finite", who, hand_distance);
    return -1;
  }
  for (int i = 0; i < 3; ++i) {
    if (!finite(tip_offset[i])) {
      set_error("%s: tip_offset[%d]=%g is not finite", who, i, tip_offset[i]);
      return -1;
    }
  }
  const int rc = launch_hull_place(verts, vert_offset, M, directions, A, hand_distance, tip_offset, status, base_pos, base_rot, simplex, t,
                                   static_cast<hipStream_t>(stream));
  if (rc < 0) return rc;
  g_hull_launches.add(0, 1);
  g_hull_launches.add(1, rc);
  return 0;
}

int a3vt_hull_place_launches(long long *counts, int reset) { return g_hull_launches.read(counts, reset); }

// ---- mesh and point-cloud rendering (scene_render.hip) -----------------------------------------------------------------------------
namespace {
LaunchCounts<2> g_scene_launches;

// One HOST offset table of M + 1 entries against its primitive table of `count` rows.
int scene_offsets_check(const char *name, const int32_t *offset, int M, int count, const char *table) {
  if (offset[0] < 0) {
    set_error("scene_render: %s[0]=%d is below 0", name, (int)offset[0]);
    return -1;
  }
  for (int m = 0; m < M; ++m) {
    if (offset[m + 1] < offset[m]) {
      set_error("scene_render: %s[%d]=%d is below %s[%d]=%d: offsets must not decrease", name, m + 1, (int)offset[m + 1], name, m,
                (int)offset[m]);
      return -1;
    }
  }
  if (offset[M] > count) {
    set_error("scene_render: %s[%d]=%d runs past %s=%d", name, M, (int)offset[M], table, count);
    return -1;
  }
  return 0;
}
}  // namespace

int a3vt_scene_render(const float *verts, int V, const int32_t *faces, const uint8_t *face_rgb, int F, const float *centres,
                      const float *radii, const uint8_t *sphere_rgb, int S, const int32_t *face_offset, const int32_t *sphere_offset,
                      int M, const int32_t *image_scene, const float *cam_pos, const float *cam_rot, int I, float yfov, float znear,
                      float zfar, int W, int H, const float *lights, int L, float ambient, const uint8_t *background, uint8_t *rgb,
                      float *depth, int32_t *prim, void *stream) {
  const char *who = "scene_render";
  if (check_range(who, "I", I, 1, kSceneMaxImages) || check_range(who, "M", M, 1, kSceneMaxScenes) ||
      check_range(who, "W", W, 1, kSceneMaxSide) || check_range(who, "H", H, 1, kSceneMaxSide) ||
      check_range(who, "L", L, 0, kSceneMaxLights) || check_range(who, "V", V, 0, kSceneMaxIndex) ||
      check_range(who, "F", F, 0, kSceneMaxIndex) || check_range(who, "S", S, 0, kSceneMaxIndex))
    return -1;
  if (!(yfov > 0.f && (double)yfov < 3.14159265358979323846)) {
    set_error("%s: yfov=%g outside (0, pi)", who, (double)yfov);
    return -1;
  }
  if (!(znear > 0.f)) {
    set_error("%s: znear=%g must be > 0", who, (double)znear);
    return -1;
  }
  if (!(znear < zfar && zfar <= 3.402823466e38f)) {
    set_error("%s: zfar=%g must be finite and above znear=%g", who, (double)zfar, (double)znear);
    return -1;
  }
  if (!(ambient >= -3.402823466e38f && ambient <= 3.402823466e38f)) {
    set_error("%s: ambient=%g must be finite", who, (double)ambient);
    return -1;
  }
  if (check_ptrs(who, {{"verts", verts, V > 0, 4, "required when V > 0"},
                       {"faces", faces, F > 0, 4, "required when F > 0"},
                       {"face_rgb", face_rgb, F > 0, 1, "required when F > 0"},
                       {"centres", centres, S > 0, 4, "required when S > 0"},
                       {"radii", radii, S > 0, 4, "required when S > 0"},
                       {"sphere_rgb", sphere_rgb, S > 0, 1, "required when S > 0"},
                       {"face_offset", face_offset, true, 4, "required (a host table)"},
                       {"sphere_offset", sphere_offset, true, 4, "required (a host table)"},
                       {"image_scene", image_scene, true, 4, "required (a host table)"},
                       {"cam_pos", cam_pos, true, 4, "required"},
                       {"cam_rot", cam_rot, true, 4, "required"},
                       {"lights", lights, L > 0, 4, "required when L > 0 (a host table)"},
                       {"background", background, true, 1, "required (a host table)"},
                       {"rgb", rgb, true, 1, "required"},
                       {"depth", depth, true, 4, "required"},
                       {"prim", prim, false, 4, ""}}))
    return -1;
  // the host tables' contents
  if (scene_offsets_check("face_offset", face_offset, M, F, "F") || scene_offsets_check("sphere_offset", sphere_offset, M, S, "S")) return -1;
  for (int i = 0; i < I; ++i) {
    if (image_scene[i] < 0 || image_scene[i] >= M) {
      set_error("%s: image_scene[%d]=%d outside 0..%d", who, i, (int)image_scene[i], M - 1);
      return -1;
    }
  }
  SceneRange *ranges = static_cast<SceneRange *>(malloc(sizeof(SceneRange) * (size_t)I));
  if (!ranges) {
    set_error("%s: no host memory for the ranges of I=%d images", who, I);
    return -1;
  }
  for (int i = 0; i < I; ++i) {
    const int m = image_scene[i];
    ranges[i] = {face_offset[m], face_offset[m + 1], sphere_offset[m], sphere_offset[m + 1]};
  }
  const int rc = launch_scene_render(verts, V, faces, face_rgb, F, centres, radii, sphere_rgb, ranges, cam_pos, cam_rot, I, yfov, znear,
                                     zfar, W, H, lights, L, ambient, background, rgb, depth, prim, static_cast<hipStream_t>(stream));
  free(ranges);
  if (rc < 0) return rc;
  g_scene_launches.add(0, 1);
  g_scene_launches.add(1, rc);
  return 0;
}

int a3vt_scene_launches(long long *counts, int reset) { return g_scene_launches.read(counts, reset); }

// ---- scenes of posed instances (posed_render.hip) ------------------------------------------------------------------------------------
namespace {
LaunchCounts<3> g_posed_launches;

// One HOST offset table of n + 1 entries against its table of `count` rows (scene_offsets_check under another name in the message).
int posed_offsets_check(const char *who, const char *name, const int32_t *offset, int n, int count, const char *table) {
  if (offset[0] < 0) {
    set_error("%s: %s[0]=%d is below 0", who, name, (int)offset[0]);
    return -1;
  }
  for (int m = 0; m < n; ++m) {
    if (offset[m + 1] < offset[m]) {
      set_error("%s: %s[%d]=%d is below %s[%d]=%d: offsets must not decrease", who, name, m + 1, (int)offset[m + 1], name, m,
                (int)offset[m]);
      return -1;
    }
  }
  if (offset[n] > count) {
    set_error("%s: %s[%d]=%d runs past %s=%d", who, name, n, (int)offset[n], table, count);
    return -1;
  }
  return 0;
}
}  // namespace

int a3vt_scene_render_posed(const float *part_verts, int PV, const int32_t *part_faces, int PF, const int32_t *part_face_offset,
                            const float *part_bound, int P, const int32_t *inst_part, const float *inst_pos, const float *inst_rot,
                            const uint8_t *inst_rgb, int N, const int32_t *inst_offset, const float *cam_pos, const float *cam_rot, int I,
                            float yfov, float znear, float zfar, int W, int H, const float *lights, int L, float ambient,
                            const uint8_t *background, uint8_t *rgb, float *depth, int32_t *prim_inst, int32_t *prim_face, void *stream) {
  const char *who = "scene_render_posed";
  if (check_range(who, "I", I, 1, kSceneMaxImages) || check_range(who, "P", P, 1, kPosedMaxParts) ||
      check_range(who, "W", W, 1, kSceneMaxSide) || check_range(who, "H", H, 1, kSceneMaxSide) ||
      check_range(who, "L", L, 0, kSceneMaxLights) || check_range(who, "PV", PV, 0, kSceneMaxIndex) ||
      check_range(who, "PF", PF, 0, kSceneMaxIndex) || check_range(who, "N", N, 0, kPosedMaxInstances))
    return -1;
  if (!(yfov > 0.f && (double)yfov < 3.14159265358979323846)) {
    set_error("%s: yfov=%g outside (0, pi)", who, (double)yfov);
    return -1;
  }
  if (!(znear > 0.f)) {
    set_error("%s: znear=%g must be > 0", who, (double)znear);
    return -1;
  }
  if (!(znear < zfar && zfar <= 3.402823466e38f)) {
    set_error("%s: zfar=%g must be finite and above znear=%g", who, (double)zfar, (double)znear);
    return -1;
  }
  if (!(ambient >= -3.402823466e38f && ambient <= 3.402823466e38f)) {
    set_error("%s: ambient=%g must be finite", who, (double)ambient);
    return -1;
  }
  if (check_ptrs(who, {{"part_verts", part_verts, PV > 0, 4, "required when PV > 0"},
                       {"part_faces", part_faces, PF > 0, 4, "required when PF > 0"},
                       {"part_face_offset", part_face_offset, true, 4, "required (a host table)"},
                       {"part_bound", part_bound, true, 4, "required (a host table)"},
                       {"inst_part", inst_part, N > 0, 4, "required when N > 0"},
                       {"inst_pos", inst_pos, N > 0, 4, "required when N > 0"},
                       {"inst_rot", inst_rot, N > 0, 4, "required when N > 0"},
                       {"inst_rgb", inst_rgb, N > 0, 1, "required when N > 0"},
                       {"inst_offset", inst_offset, true, 4, "required (a host table)"},
                       {"cam_pos", cam_pos, true, 4, "required"},
                       {"cam_rot", cam_rot, true, 4, "required"},
                       {"lights", lights, L > 0, 4, "required when L > 0 (a host table)"},
                       {"background", background, true, 1, "required (a host table)"},
                       {"rgb", rgb, true, 1, "required"},
                       {"depth", depth, true, 4, "required"},
                       {"prim_inst", prim_inst, prim_face != nullptr, 4, "required when prim_face is given"},
                       {"prim_face", prim_face, prim_inst != nullptr, 4, "required when prim_inst is given"}}))
    return -1;
  // the host tables' contents
  if (posed_offsets_check(who, "part_face_offset", part_face_offset, P, PF, "PF") ||
      posed_offsets_check(who, "inst_offset", inst_offset, I, N, "N"))
    return -1;
  for (int p = 0; p < P; ++p) {
    for (int k = 0; k < 4; ++k) {
      const float x = part_bound[4 * p + k];
      if (!(x >= (k == 3 ? 0.f : -3.402823466e38f) && x <= 3.402823466e38f)) {
        set_error("%s: part_bound[%d][%d]=%g must be finite%s", who, p, k, (double)x, k == 3 ? " and not below 0" : "");
        return -1;
      }
    }
  }
  const int rc = launch_scene_render_posed(part_verts, PV, part_faces, part_face_offset, part_bound, P, inst_part, inst_pos, inst_rot,
                                           inst_rgb, inst_offset, cam_pos, cam_rot, I, yfov, znear, zfar, W, H, lights, L, ambient,
                                           background, rgb, depth, prim_inst, prim_face, static_cast<hipStream_t>(stream));
  if (rc < 0) return rc;
  g_posed_launches.add(0, 1);
  g_posed_launches.add(1, rc);
  return 0;
}

int a3vt_pose_parts(const float *part_verts, int PV, const int32_t *part_faces, int PF, const int32_t *part_vert_offset,
                    const int32_t *part_face_offset, int P, const int32_t *inst_part, const float *inst_pos, const float *inst_rot,
                    const uint8_t *inst_rgb, int N, const int32_t *vert_base, const int32_t *face_base, float *verts_out, int TV,
                    int32_t *faces_out, uint8_t *face_rgb_out, int TF, void *stream) {
  const char *who = "pose_parts";
  if (check_range(who, "P", P, 1, kPosedMaxParts) || check_range(who, "PV", PV, 0, kSceneMaxIndex) ||
      check_range(who, "PF", PF, 0, kSceneMaxIndex) || check_range(who, "N", N, 0, kPosedMaxInstances) ||
      check_range(who, "TV", TV, 0, kSceneMaxIndex) || check_range(who, "TF", TF, 0, kSceneMaxIndex))
    return -1;
  if (check_ptrs(who, {{"part_verts", part_verts, PV > 0, 4, "required when PV > 0"},
                       {"part_faces", part_faces, PF > 0, 4, "required when PF > 0"},
                       {"part_vert_offset", part_vert_offset, true, 4, "required (a host table)"},
                       {"part_face_offset", part_face_offset, true, 4, "required (a host table)"},
                       {"inst_part", inst_part, N > 0, 4, "required when N > 0"},
                       {"inst_pos", inst_pos, N > 0, 4, "required when N > 0"},
                       {"inst_rot", inst_rot, N > 0, 4, "required when N > 0"},
                       {"inst_rgb", inst_rgb, N > 0, 1, "required when N > 0"},
                       {"vert_base", vert_base, N > 0, 4, "required when N > 0"},
                       {"face_base", face_base, N > 0, 4, "required when N > 0"},
                       {"verts_out", verts_out, TV > 0, 4, "required when TV > 0"},
                       {"faces_out", faces_out, TF > 0, 4, "required when TF > 0"},
                       {"face_rgb_out", face_rgb_out, TF > 0, 1, "required when TF > 0"}}))
    return -1;
  if (posed_offsets_check(who, "part_vert_offset", part_vert_offset, P, PV, "PV") ||
      posed_offsets_check(who, "part_face_offset", part_face_offset, P, PF, "PF"))
    return -1;
  const int rc = launch_pose_parts(part_verts, part_faces, part_vert_offset, part_face_offset, P, inst_part, inst_pos, inst_rot, inst_rgb,
                                   N, vert_base, face_base, verts_out, TV, faces_out, face_rgb_out, TF, static_cast<hipStream_t>(stream));
  if (rc < 0) return rc;
  g_posed_launches.add(2, rc);
  return 0;
}

int a3vt_posed_launches(long long *counts, int reset) { return g_posed_launches.read(counts, reset); }

// ---- the ground-truth point cloud of a batch of meshes (voxel.hip) -----------------------------------------------------------------
namespace {
LaunchCounts<3> g_voxel_launches;

int voxel_size_check(const char *who, int M, int dim) {
  if (check_range(who, "dim", dim, kVoxelMinDim, kVoxelMaxDim) || check_range(who, "M", M, 1, kVoxelMaxMeshes)) return -1;
  if ((long long)M * dim * dim * dim > kVoxelMaxCells) {
    set_error("%s: M=%d meshes at dim=%d are more than %lld voxels", who, M, dim, kVoxelMaxCells);
    return -1;
  }
  return 0;
}
}  // namespace

int a3vt_voxel_surface(const float *verts, int V, const int32_t *faces, int F, const int32_t *vert_offset, const int32_t *face_offset, int M,
                       int dim, uint8_t *occupancy, int32_t *depth_maps, int32_t *counts, void *stream) {
  if (voxel_size_check("voxel_surface", M, dim)) return -1;
  if (check_range("voxel_surface", "V", V, 0, kVoxelMaxIndex) || check_range("voxel_surface", "F", F, 0, kVoxelMaxIndex)) return -1;
  if (check_ptrs("voxel_surface", {{"verts", verts, V > 0, 4, "required when V > 0"},
                                   {"faces", faces, F > 0, 4, "required when F > 0"},
                                   {"vert_offset", vert_offset, true, 4, "required"},
                                   {"face_offset", face_offset, true, 4, "required"},
                                   {"occupancy", occupancy, false, 1, ""},
                                   {"depth_maps", depth_maps, false, 4, ""},
                                   {"counts", counts, true, 4, "required"}}))
    return -1;
  const int rc = launch_voxel_surface(verts, V, faces, F, vert_offset, face_offset, M, dim, occupancy, depth_maps, counts,
                                      static_cast<hipStream_t>(stream));
  if (rc < 0) return rc;
  g_voxel_launches.add(0, rc);
  return 0;
}

int a3vt_voxel_depth_maps(const uint8_t *voxels, int M, int dim, int32_t *depth_maps, void *stream) {
  if (voxel_size_check("voxel_depth_maps", M, dim)) return -1;
  if (check_ptrs("voxel_depth_maps", {{"voxels", voxels, true, 1, "required"}, {"depth_maps", depth_maps, true, 4, "required"}})) return -1;
  const int rc = launch_voxel_depth_maps(voxels, M, dim, depth_maps, static_cast<hipStream_t>(stream));
  if (rc < 0) return rc;
  g_voxel_launches.add(1, rc);
  return 0;
}

int a3vt_voxel_points(int M, int dim, long long total, int32_t *surface, float *aligned, const long long *index, int num_points, float *cloud,
                      void *stream) {
  if (voxel_size_check("voxel_points", M, dim)) return -1;
  if (check_range("voxel_points", "total", total, 0, kVoxelMaxCells)) return -1;
  if (cloud && check_range("voxel_points", "num_points", num_points, 1, kVoxelMaxIndex)) return -1;
  if (check_ptrs("voxel_points", {{"surface", surface, total > 0, 4, "required when total > 0"},
                                  {"aligned", aligned, false, 4, ""},
                                  {"index", index, cloud != nullptr, 8, "index and cloud go together"},
                                  {"cloud", cloud, index != nullptr, 4, "index and cloud go together"}}))
    return -1;
  const int rc = launch_voxel_points(M, dim, total, surface, aligned, index, num_points, cloud, static_cast<hipStream_t>(stream));
  if (rc < 0) return rc;
  g_voxel_launches.add(2, rc);
  return 0;
}

int a3vt_voxel_launches(long long *counts, int reset) { return g_voxel_launches.read(counts, reset); }

// ---- the supervised latent policy's value network (latent_policy.hip) ------------------------------------------------------------
namespace {
static_assert(sizeof(a3vt_mlp) == sizeof(PolicyNet) && sizeof(a3vt_mlp_layer) == sizeof(PolicyLayer) &&
                  sizeof(a3vt_mlp_grads) == sizeof(PolicyGrads) && offsetof(a3vt_mlp, n_layers) == offsetof(PolicyNet, n_layers) &&
                  offsetof(a3vt_mlp, scale) == offsetof(PolicyNet, scale) && offsetof(a3vt_mlp_layer, in) == offsetof(PolicyLayer, in),
              "a3vt_mlp is PolicyNet field for field");
LaunchCounts<3> g_policy_launches;

// The table's own rules -> floats of a stash row (the sum of the layers' out), or -1 with the message set.
int policy_net_check(const char *who, const a3vt_mlp *net) {
  if (!net) {
    set_error("%s: net is null", who);
    return -1;
  }
  if (net->n_layers < 2 || net->n_layers > kPolicyMaxLayers || net->concat_at < 1 || net->concat_at >= net->n_layers ||
      net->latent_size < 1 || 3 * (long long)net->latent_size > kPolicyMaxWidth || (net->transform != 0 && net->transform != 1)) {
    set_error("%s: n_layers=%d (2..%d) concat_at=%d (1..n_layers-1) latent_size=%d (3*latent_size <= %d) transform=%d (0, 1) unsupported",
              who, net->n_layers, kPolicyMaxLayers, net->concat_at, net->latent_size, kPolicyMaxWidth, net->transform);
    return -1;
  }
  int total = 0;
  for (int l = 0; l < net->n_layers; ++l) {
    const a3vt_mlp_layer &L = net->layer[l];
    if (L.in < 1 || L.in > kPolicyMaxWidth || L.out < 1 || L.out > kPolicyMaxWidth) {
      set_error("%s: layer %d in=%d out=%d outside 1..%d", who, l, L.in, L.out, kPolicyMaxWidth);
      return -1;
    }
    const int want = l == 0 ? L.in : net->layer[l - 1].out + (l == net->concat_at ? 2 * net->latent_size : 0);
    if (L.in != want) {
      set_error("%s: layer %d in=%d does not chain (the rows before it give %d)", who, l, L.in, want);
      return -1;
    }
    if (!L.weight || !L.bias || !aligned_to(L.weight, L.in % 4 == 0 ? 16 : 4) || !aligned_to(L.bias, 4)) {
      set_error("%s: layer %d weight / bias null or misaligned (weight: %d bytes)", who, l, L.in % 4 == 0 ? 16 : 4);
      return -1;
    }
    total += L.out;
  }
  return total;
}
PolicyNet policy_net_of(const a3vt_mlp *net) {
  PolicyNet n;
  memcpy(&n, net, sizeof(n));
  return n;
}
}  // namespace

int a3vt_latent_policy_limit(int which) {
  return which == 0 ? kPolicyMaxRows : which == 1 ? kPolicyMaxWidth : which == 2 ? kPolicyMaxLayers : 0;
}

int a3vt_latent_policy_stash_floats(const a3vt_mlp *net) {
  const int total = policy_net_check("latent_policy_stash_floats", net);
  return total < 0 ? 0 : total;
}

int a3vt_latent_policy_fwd(const a3vt_mlp *net, const float *mask, const float *latent, const float *first_latent, const float *taken,
                           int rows, float *values, int32_t *action, float *stash, void *stream) {
  const int ld = policy_net_check("latent_policy_fwd", net);
  if (ld < 0 || check_count("latent_policy_fwd", "rows", rows, kPolicyMaxRows)) return -1;
  A3VT_CHECK_ARG(mask && latent && first_latent && values);
  A3VT_CHECK_ARG((taken && action) || (!taken && !action));
  A3VT_CHECK_ARG(aligned_to(mask, 4) && aligned_to(latent, 4) && aligned_to(first_latent, 4) && aligned_to(taken, 4) &&
                 aligned_to(values, 4) && aligned_to(action, 4) && aligned_to(stash, 4));
  g_policy_launches.add(0, 1);
  return launch_policy_fwd(policy_net_of(net), mask, latent, first_latent, taken, rows, values, action, stash, ld,
                           static_cast<hipStream_t>(stream));
}

int a3vt_action_value_loss(const float *values, const int32_t *actions, const float *targets, int steps, int rows, int num_actions,
                           float *loss, float *dvalues, void *stream) {
  if (check_count("action_value_loss", "steps", steps, kPolicyMaxRows) || check_count("action_value_loss", "rows", rows, kPolicyMaxRows) ||
      check_count("action_value_loss", "num_actions", num_actions, kPolicyMaxWidth))
    return -1;
  A3VT_CHECK_ARG(values && actions && targets && loss && dvalues);
  A3VT_CHECK_ARG(aligned_to(values, 4) && aligned_to(actions, 4) && aligned_to(targets, 4) && aligned_to(loss, 4) && aligned_to(dvalues, 4));
  g_policy_launches.add(1, 1);
  return launch_action_value_loss(values, actions, targets, steps, rows, num_actions, loss, dvalues, static_cast<hipStream_t>(stream));
}

int a3vt_latent_policy_bwd(const a3vt_mlp *net, const a3vt_mlp_grads *grads, const float *mask, const float *latent,
                           const float *first_latent, const float *dvalues, const float *stash, float *delta, int rows, int accumulate,
                           void *stream) {
  const int ld = policy_net_check("latent_policy_bwd", net);
  if (ld < 0 || check_count("latent_policy_bwd", "rows", rows, kPolicyMaxRows)) return -1;
  A3VT_CHECK_ARG(grads && mask && latent && first_latent && dvalues && stash && delta);
  A3VT_CHECK_ARG(aligned_to(mask, 4) && aligned_to(latent, 4) && aligned_to(first_latent, 4) && aligned_to(dvalues, 4) &&
                 aligned_to(stash, 4) && aligned_to(delta, 4));
  PolicyGrads g;
  memcpy(&g, grads, sizeof(g));
  if (check_grads("latent_policy_bwd", g, net->n_layers)) return -1;
  g_policy_launches.add(2, 2);
  return launch_policy_bwd(policy_net_of(net), g, mask, latent, first_latent, dvalues, stash, delta, rows, ld, accumulate ? 1 : 0,
                           static_cast<hipStream_t>(stream));
}

int a3vt_latent_policy_launches(long long *counts, int reset) { return g_policy_launches.read(counts, reset); }

// ---- DDQN's Latent_Model on the same layer table (ddqn_latent.hip) ---------------------------------------------------------------
namespace {
LaunchCounts<2> g_ddqn_latent_launches;

// The table's rules plus the learner's: transform 0, at most kTdMaxActions outputs -> floats of a stash row, or -1 (message set).
int ddqn_latent_net_check(const char *who, const a3vt_mlp *net) {
  const int ld = policy_net_check(who, net);
  if (ld < 0) return -1;
  const int A = net->layer[net->n_layers - 1].out;
  if (net->transform != 0 || A > kTdMaxActions) {
    set_error("%s: transform=%d (0: a Q network has no output squashing) num_actions=%d (1..%d) unsupported", who, net->transform, A,
              kTdMaxActions);
    return -1;
  }
  return ld;
}
}  // namespace

size_t a3vt_ddqn_latent_scratch_bytes(const a3vt_mlp *online, int batch) {
  const int ld = ddqn_latent_net_check("ddqn_latent_scratch_bytes", online);
  if (ld < 0 || check_count("ddqn_latent_scratch_bytes", "batch", batch, kTdMaxBatch)) return 0;
  return (size_t)batch * (2 * (size_t)online->layer[online->n_layers - 1].out + 2 * (size_t)ld) * sizeof(float);
}

int a3vt_ddqn_latent_q(const a3vt_mlp *net, const float *mask, const float *latent, const float *first_latent, const float *mask_penalty,
                       int rows, float *q, int32_t *action, void *stream) {
  if (ddqn_latent_net_check("ddqn_latent_q", net) < 0 || check_count("ddqn_latent_q", "rows", rows, kTdMaxBatch)) return -1;
  A3VT_CHECK_ARG(mask && latent && first_latent && q);
  A3VT_CHECK_ARG((mask_penalty && action) || (!mask_penalty && !action));
  A3VT_CHECK_ARG(aligned_to(mask, 4) && aligned_to(latent, 4) && aligned_to(first_latent, 4) && aligned_to(mask_penalty, 4) &&
                 aligned_to(q, 4) && aligned_to(action, 4));
  g_ddqn_latent_launches.add(0, 1);
  return launch_ddqn_latent_q(policy_net_of(net), mask, latent, first_latent, mask_penalty, rows, q, action, static_cast<hipStream_t>(stream));
}

int a3vt_ddqn_latent_update(const a3vt_mlp *online, const a3vt_mlp *target_net, const a3vt_mlp_grads *grads, const float *mask,
                            const float *mask_n, const float *latent, const float *latent_n, const float *first_latent,
                            const float *actions, const float *rewards, const float *denom, int batch, int budget, float gamma,
                            float *q_cur, int32_t *best_next, float *target, float *diff, float *loss, void *scratch, void *stream) {
  const int ld = ddqn_latent_net_check("ddqn_latent_update (online)", online);
  if (ld < 0 || ddqn_latent_net_check("ddqn_latent_update (target)", target_net) < 0 ||
      check_count("ddqn_latent_update", "batch", batch, kTdMaxBatch))
    return -1;
  if (online->n_layers != target_net->n_layers || online->concat_at != target_net->concat_at ||
      online->latent_size != target_net->latent_size) {
    set_error("ddqn_latent_update: the target net has n_layers=%d concat_at=%d latent_size=%d, the online net %d %d %d", target_net->n_layers,
              target_net->concat_at, target_net->latent_size, online->n_layers, online->concat_at, online->latent_size);
    return -1;
  }
  if (online->layer[0].in != online->layer[online->n_layers - 1].out) {   // (mask is the network's input AND the table of taken actions)
    set_error("ddqn_latent_update: layer 0 in=%d is not num_actions=%d (mask feeds the network and penalises the actions)",
              online->layer[0].in, online->layer[online->n_layers - 1].out);
    return -1;
  }
  for (int l = 0; l < online->n_layers; ++l) {
    const a3vt_mlp_layer &a = online->layer[l], &b = target_net->layer[l];
    if (a.in != b.in || a.out != b.out || (a.relu != 0) != (b.relu != 0)) {
      set_error("ddqn_latent_update: layer %d of the target net is in=%d out=%d relu=%d, of the online net in=%d out=%d relu=%d", l, b.in, b.out,
                b.relu, a.in, a.out, a.relu);
      return -1;
    }
  }
  A3VT_CHECK_ARG(grads && mask && mask_n && latent && latent_n && first_latent && actions && rewards);
  A3VT_CHECK_ARG(q_cur && best_next && target && diff && loss && scratch);
  A3VT_CHECK_ARG(aligned_to(mask, 4) && aligned_to(mask_n, 4) && aligned_to(latent, 4) && aligned_to(latent_n, 4) &&
                 aligned_to(first_latent, 4) && aligned_to(actions, 4) && aligned_to(rewards, 4) && aligned_to(denom, 4));
  A3VT_CHECK_ARG(aligned_to(q_cur, 4) && aligned_to(best_next, 4) && aligned_to(target, 4) && aligned_to(diff, 4) && aligned_to(loss, 4) &&
                 aligned_to(scratch, 4));
  PolicyGrads g;
  memcpy(&g, grads, sizeof(g));
  if (check_grads("ddqn_latent_update", g, online->n_layers)) return -1;
  DdqnLatentArgs a{};
  a.mask = mask, a.mask_n = mask_n, a.latent = latent, a.latent_n = latent_n, a.first_latent = first_latent;
  a.actions = actions, a.rewards = rewards, a.denom = denom;
  a.batch = batch, a.budget = budget, a.ld = ld, a.gamma = gamma;
  a.q_cur = q_cur, a.diff = diff, a.target = target, a.loss = loss, a.best_next = best_next;
  a.scratch = static_cast<float *>(scratch);
  g_ddqn_latent_launches.add(1, 3);
  return launch_ddqn_latent_update(policy_net_of(online), policy_net_of(target_net), g, a, static_cast<hipStream_t>(stream));
}

int a3vt_ddqn_latent_launches(long long *counts, int reset) { return g_ddqn_latent_launches.read(counts, reset); }

namespace {
struct QnetLayout {
  size_t za, heavy, ga, dz, db_slab, slab, total;
  int ldza;   // as LayerLayout's
};
QnetLayout qnet_layout(int batch, int n_vert, int hidden, int cut_len, int backward) {
  QnetLayout L{};
  const size_t m = (size_t)batch * n_vert;
  const int npad = pad4(hidden);
  L.ldza = pad4(cut_len) > 4 ? pad4(cut_len) : 4;
  Arena a;
  L.za = a.take(m * L.ldza);
  L.heavy = a.take(csr_heavy_scratch_ints(n_vert));
  if (backward) {
    L.ga = a.take(m * L.ldza);
    L.dz = a.take(m * npad);
    L.db_slab = a.take((size_t)csr_bwd_num_slabs(batch, n_vert) * L.ldza);
    L.slab = a.take((size_t)qnet_bwd_wgs(batch, n_vert) * qnet_slab_floats(hidden));
  }
  L.total = a.off;
  return L;
}
int check_qnet_dims(int hidden, int cut_len, int n_vert, int batch) {
  if (hidden < 1 || hidden > 304 || cut_len < 0 || cut_len > hidden) {
    set_error("qnet_input: hidden=%d (1..304) cut_len=%d unsupported", hidden, cut_len);
    return -1;
  }
  if (n_vert < 1 || batch < 1 || (long long)batch * ((n_vert + 63) / 64) > 0x7fffffffll) {
    set_error("qnet_input: batch=%d n_vert=%d unsupported", batch, n_vert);
    return -1;
  }
  return 0;
}
}  // namespace

size_t a3vt_qnet_input_scratch_bytes(int batch, int n_vert, int hidden, int cut_len, int backward) {
  if (batch < 1 || n_vert < 1 || hidden < 1 || hidden > 304 || cut_len < 0 || cut_len > hidden) return 0;
  return qnet_layout(batch, n_vert, hidden, cut_len, backward).total * sizeof(float);
}

int a3vt_qnet_input_fwd(const float *mesh, const float *w1, const float *b1, const float *w2, const float *b2, const float *comp_s,
                        const float *comp_t, const float *comp_c, const float *bias, int hidden, int cut_len, const int32_t *rowptr,
                        const int32_t *col, const float *val, int max_degree, int n_vert, int batch, float *y, int ld_y,
                        float *scratch, void *stream) {
  if (int rc = check_qnet_dims(hidden, cut_len, n_vert, batch)) return rc;
  A3VT_CHECK_ARG(mesh && w1 && b1 && w2 && b2 && comp_s && comp_t && comp_c && bias && rowptr && col && val && y && scratch);
  A3VT_CHECK_ARG(ld_y % 4 == 0 && ld_y >= hidden);
  A3VT_CHECK_ARG(aligned_to(mesh, 16) && aligned_to(comp_s, 16) && aligned_to(comp_t, 16) && aligned_to(comp_c, 16) && aligned_to(scratch, 16));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const QnetLayout L = qnet_layout(batch, n_vert, hidden, cut_len, 0);
  QnetArgs a{};
  a.mesh = mesh;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.comp_s = comp_s; a.comp_t = comp_t; a.comp_c = comp_c;
  a.batch = batch; a.n_vert = n_vert; a.hidden = hidden; a.cut_len = cut_len;
  a.za = scratch + L.za;
  a.ldza = L.ldza;
  a.y = y;
  a.ldy = ld_y;
  path_count(PATH_QNET_FWD);
  if (int rc = launch_qnet_fwd(a, s)) return rc;
  return layer_fwd_tail(a.za, a.ldza, bias, cut_len, 1, rowptr, col, val, max_degree, n_vert, batch, y, ld_y, scratch + L.heavy, s);
}

int a3vt_qnet_input_bwd(const float *mesh, const float *w1, const float *b1, const float *w2, const float *b2, const float *comp_c,
                        int hidden, int cut_len, const int32_t *rowptrT, const int32_t *colT, const float *valT, int max_degreeT,
                        int n_vert, int batch, const float *y, int ld_y, const float *grad_y, int ld_gy, float *d_s, float *d_t,
                        float *d_c, float *dw1, float *db1, float *dw2, float *db2, float *grad_bias, float *scratch, void *stream) {
  if (int rc = check_qnet_dims(hidden, cut_len, n_vert, batch)) return rc;
  A3VT_CHECK_ARG(mesh && w1 && b1 && w2 && b2 && comp_c && rowptrT && colT && valT && y && grad_y && scratch);
  A3VT_CHECK_ARG(d_s && d_t && d_c && dw1 && db1 && dw2 && db2 && grad_bias);
  A3VT_CHECK_ARG(ld_y >= hidden && ld_gy >= hidden);
  A3VT_CHECK_ARG(aligned_to(mesh, 16) && aligned_to(comp_c, 16) && aligned_to(scratch, 16));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const QnetLayout L = qnet_layout(batch, n_vert, hidden, cut_len, 1);
  float *dz = scratch + L.dz;
  path_count(PATH_QNET_BWD);
  if (int rc = layer_bwd_tail(grad_y, ld_gy, y, ld_y, 1, hidden, cut_len, rowptrT, colT, valT, max_degreeT, n_vert, batch,
                              scratch + L.ga, dz, scratch + L.db_slab, scratch + L.heavy, grad_bias, s))
    return rc;
  QnetArgs a{};
  a.mesh = mesh;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.comp_c = comp_c;
  a.batch = batch; a.n_vert = n_vert; a.hidden = hidden; a.cut_len = cut_len;
  a.dz = dz;
  a.slab = scratch + L.slab;
  return launch_qnet_bwd(a, d_s, d_t, d_c, dw1, db1, dw2, db2, s);
}

// ---- FoldingNet fold (fold.hip) ----------------------------------------------------------------------------------------------
size_t a3vt_fold_workspace_bytes(int batch, int points, int backward) { return fold_workspace_bytes(batch, points, backward); }

int a3vt_fold_fwd(const float *bias_s, const float *g, int k, const float *w1g, const float *w2, const float *b2, const float *w3,
                  const float *b3, int batch, int points, int width, float *y, void *workspace, size_t workspace_bytes, void *stream) {
  A3VT_CHECK_ARG(width == 512);
  A3VT_CHECK_ARG(k == 2 || k == 3);
  A3VT_CHECK_ARG(batch > 0 && points > 0 && (long long)batch * points <= 16000000);
  A3VT_CHECK_ARG(bias_s && g && w1g && w2 && b2 && w3 && b3 && y && workspace);
  A3VT_CHECK_ARG(aligned_to(bias_s, 16) && aligned_to(w2, 16) && aligned_to(b2, 16) && aligned_to(w3, 16) && aligned_to(workspace, 16));
  A3VT_CHECK_ARG(aligned_to(g, 4) && aligned_to(w1g, 4) && aligned_to(b3, 4) && aligned_to(y, 4));
  A3VT_CHECK_ARG(workspace_bytes >= fold_workspace_bytes(batch, points, 0));
  return launch_fold_fwd(bias_s, g, k, w1g, w2, b2, w3, b3, batch, points, y, static_cast<float *>(workspace),
                         static_cast<hipStream_t>(stream));
}

int a3vt_fold_bwd(const float *bias_s, const float *g, int k, const float *w1g, const float *w2, const float *b2, const float *w3,
                  const float *dy, int batch, int points, int width, float *d_bias_s, float *dg, float *dw1g, float *dw2, float *db2,
                  float *dw3, float *db3, void *workspace, size_t workspace_bytes, void *stream) {
  A3VT_CHECK_ARG(width == 512);
  A3VT_CHECK_ARG(k == 2 || k == 3);
  A3VT_CHECK_ARG(batch > 0 && points > 0 && (long long)batch * points <= 16000000);
  A3VT_CHECK_ARG(bias_s && g && w1g && w2 && b2 && w3 && dy && workspace);
  A3VT_CHECK_ARG(d_bias_s && dw1g && dw2 && db2 && dw3 && db3);
  A3VT_CHECK_ARG(dg == nullptr || k == 3);   // the lattice of fold 1 has no gradient
  A3VT_CHECK_ARG(aligned_to(bias_s, 16) && aligned_to(w2, 16) && aligned_to(b2, 16) && aligned_to(w3, 16) && aligned_to(workspace, 16) &&
                 aligned_to(dw2, 16));
  A3VT_CHECK_ARG(aligned_to(g, 4) && aligned_to(w1g, 4) && aligned_to(dy, 4) && aligned_to(d_bias_s, 4) && aligned_to(dg, 4) &&
                 aligned_to(dw1g, 4) && aligned_to(db2, 4) && aligned_to(dw3, 4) && aligned_to(db3, 4));
  A3VT_CHECK_ARG(workspace_bytes >= fold_workspace_bytes(batch, points, 1));
  return launch_fold_bwd(bias_s, g, k, w1g, w2, b2, w3, dy, batch, points, d_bias_s, dg, dw1g, dw2, db2, dw3, db3,
                         static_cast<float *>(workspace), static_cast<hipStream_t>(stream));
}

int a3vt_wt_rows(int n_out) { return rowgemm_bt_rows(n_out); }
int a3vt_wt_ld(int k) { return pad16(k); }

int a3vt_transpose_weight(const float *w, int k, int n_out, float *wt, void *stream) {
  A3VT_CHECK_ARG(w && wt && k > 0 && n_out > 0 && n_out <= 304);
  return launch_transpose_pad(w, k, n_out, wt, rowgemm_bt_rows(n_out), pad16(k), static_cast<hipStream_t>(stream));
}

int a3vt_rowgemm(const float *a, int lda, int m, int k, const float *wt, int n_out, int gemm_bf16, float *c, int ldc,
                 void *stream) {
  A3VT_CHECK_ARG(a && wt && c && m > 0 && k > 0 && k % 4 == 0 && lda >= k && ldc >= n_out && n_out <= 304);
  RowGemmArgs g{};
  g.a0 = g.a1 = a;
  g.lda0 = g.lda1 = lda;
  g.ksplit = k;
  g.bt = wt;
  g.ldb = pad16(k);
  g.zeros = zero_page();
  A3VT_CHECK_ARG(g.zeros != nullptr);
  g.m = m;
  g.k = k;
  g.n_store = n_out;
  g.c = c;
  g.ldc = ldc;
  g.mode = gemm_bf16 == GEMM_BF16_OPERANDS ? GEMM_BF16_OPERANDS : GEMM_FP32;   // (mode 3 is a stack mode: a lone layer runs exact)
  return launch_rowgemm(g, EPI_PLAIN, static_cast<hipStream_t>(stream));
}

size_t a3vt_posenc_param_count(int input_size) { return posenc_param_count(input_size); }
size_t a3vt_posenc_scratch_bytes(int m, int input_size) {
  return (size_t)posenc_num_slabs(m) * posenc_param_count(input_size) * sizeof(float);
}
int a3vt_posenc_mask_fwd(const float *verts, const float *mask, int m, int input_size, const float *pe_params,
                         float *feats, int ld_feats, void *stream) {
  A3VT_CHECK_ARG(verts && mask && pe_params && feats && m > 0 && ld_feats >= input_size);
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_posenc_fwd(verts, mask, m, input_size, pe_params, feats, ld_feats, static_cast<hipStream_t>(stream));
}
int a3vt_posenc_mask_bwd(const float *verts, const float *mask, int m, int input_size, const float *pe_params,
                         const float *grad_feats, int ld_feats, float *grad_verts, float *grad_params, float *scratch,
                         void *stream) {
  // (any ld_feats >= input_size and any 4-byte-aligned grad_feats: the kernel takes 16-byte loads only where they are aligned)
  A3VT_CHECK_ARG(verts && mask && pe_params && grad_feats && grad_verts && grad_params && scratch && m > 0 &&
                 ld_feats >= input_size);
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_posenc_bwd(verts, mask, m, input_size, pe_params, grad_feats, ld_feats, grad_verts, grad_params,
                           scratch, static_cast<hipStream_t>(stream));
}

// ---- wide inputs (I = 448 of the image models): posenc_wide.hip
int a3vt_posenc_wide_supported(int input_size) { return posenc_wide_supported(input_size) ? 1 : 0; }
size_t a3vt_posenc_wide_acts_bytes(int m, int input_size) {
  return posenc_wide_supported(input_size) && m > 0 ? posenc_wide_acts_floats(m, input_size) * sizeof(float) : 0;
}
size_t a3vt_posenc_wide_scratch_bytes(int m, int input_size, int need_backward) {
  return posenc_wide_supported(input_size) && m > 0 ? posenc_wide_scratch_floats(m, input_size, need_backward) * sizeof(float) : 0;
}
int a3vt_posenc_wide_fwd(const float *verts, const float *mask, int m, int input_size, const float *pe_params, float *feats,
                         int ld_feats, float *acts, float *scratch, int gemm_bf16, void *stream) {
  A3VT_CHECK_ARG(verts && mask && pe_params && feats && acts && scratch && m > 0);
  A3VT_CHECK_ARG(posenc_wide_supported(input_size) && ld_feats == input_size);   // before anything touches the device
  const float *zeros = zero_page();
  A3VT_CHECK_ARG(zeros != nullptr);
  A3VT_CHECK_ARG(gemm_bf16 == GEMM_FP32 || gemm_bf16 == GEMM_BF16_OPERANDS);
  return launch_posenc_wide_fwd(verts, mask, m, input_size, pe_params, feats, ld_feats, acts, scratch, zeros, gemm_bf16,
                                static_cast<hipStream_t>(stream));
}
int a3vt_posenc_wide_bwd(const float *verts, const float *mask, int m, int input_size, const float *pe_params,
                         const float *grad_feats, int ld_feats, const float *acts, float *grad_verts, float *grad_params,
                         float *scratch, int gemm_bf16, void *stream) {
  A3VT_CHECK_ARG(verts && mask && pe_params && grad_feats && acts && grad_verts && grad_params && scratch && m > 0);
  A3VT_CHECK_ARG(posenc_wide_supported(input_size) && ld_feats == input_size);
  const float *zeros = zero_page();
  A3VT_CHECK_ARG(zeros != nullptr);
  A3VT_CHECK_ARG(gemm_bf16 == GEMM_FP32 || gemm_bf16 == GEMM_BF16_OPERANDS);
  return launch_posenc_wide_bwd(verts, mask, m, input_size, pe_params, grad_feats, ld_feats, acts, grad_verts, grad_params,
                                scratch, zeros, gemm_bf16, static_cast<hipStream_t>(stream));
}

int a3vt_vertex_update(const float *verts_in, const float *update, int batch, int n_vert, int n_vision,
                       float *verts_out, void *stream) {
  A3VT_CHECK_ARG(verts_in && update && verts_out && batch > 0 && n_vert > 0 && n_vision >= 0 && n_vision <= n_vert);
  return launch_vertex_update(verts_in, update, batch, n_vert, n_vision, verts_out, static_cast<hipStream_t>(stream));
}

int a3vt_face_cdf(const float *verts, const int32_t *faces, int batch, int n_vert, int n_faces, float *cdf,
                  void *stream) {
  A3VT_CHECK_ARG(verts && faces && cdf && batch > 0 && n_vert > 0 && n_faces > 0);
  return launch_face_cdf(verts, faces, batch, n_vert, n_faces, cdf, static_cast<hipStream_t>(stream));
}

int a3vt_sample_points_fwd(const float *verts, const int32_t *faces, const float *cdf, int batch, int n_vert,
                           int n_faces, int draws, int num, const int32_t *face_idx_in, const float *u_in,
                           const float *v_in, uint64_t seed, uint64_t offset, float *points, int32_t *face_idx_out,
                           float *u_out, float *v_out, void *stream) {
  A3VT_CHECK_ARG(verts && faces && points && batch > 0 && n_vert > 0 && n_faces > 0 && draws > 0 && num > 0);
  ProfScope psc(PROF_LOSS, static_cast<hipStream_t>(stream));
  return launch_sample_fwd(verts, faces, cdf, batch, n_vert, n_faces, draws, num, face_idx_in, u_in, v_in, seed,
                           offset, points, face_idx_out, u_out, v_out, static_cast<hipStream_t>(stream));
}

int a3vt_sample_points_bwd(const int32_t *faces, int batch, int n_vert, int n_faces, int draws, int num,
                           const int32_t *face_idx, const float *u, const float *v, const float *grad_points,
                           float *grad_verts, void *stream) {
  A3VT_CHECK_ARG(faces && face_idx && u && v && grad_points && grad_verts && batch > 0 && n_vert > 0 && n_faces > 0 &&
                 draws > 0 && num > 0);
  ProfScope psc(PROF_LOSS, static_cast<hipStream_t>(stream));
  return launch_sample_bwd(faces, batch, n_vert, n_faces, draws, num, face_idx, u, v, grad_points, grad_verts,
                           static_cast<hipStream_t>(stream));
}

size_t a3vt_chamfer_scratch_bytes(int draws, int batch, int p, int q) {
  (void)p;
  return draws > 0 && batch > 0 && q > 0 ? chamfer_scratch_bytes(draws, batch, q) : 0;
}

int a3vt_chamfer_fwd(const float *x, const float *y, int draws, int batch, int p, int q, float *dist_xy,
                     int32_t *idx_xy, float *dist_yx, int32_t *idx_yx, float *cd, void *scratch, void *stream) {
  A3VT_CHECK_ARG(x && y && dist_xy && idx_xy && dist_yx && idx_yx && cd);
  // brute force only: the scratch of this entry point is a3vt_chamfer_scratch_bytes() (the column minima of the sweep)
  ProfScope psc(PROF_SEARCH, static_cast<hipStream_t>(stream));
  return launch_chamfer_fwd(x, y, draws, batch, p, q, dist_xy, idx_xy, dist_yx, idx_yx, cd, scratch,
                            scratch ? a3vt_chamfer_scratch_bytes(draws, batch, p, q) : 0,
                            scratch ? NN_BRUTE_SWEEP : NN_BRUTE_TWO_PASS, static_cast<hipStream_t>(stream));
}

size_t a3vt_chamfer_workspace_bytes(int draws, int batch, int p, int q) {
  return draws > 0 && batch > 0 && p > 0 && q > 0 ? chamfer_workspace_bytes(draws, batch, p, q) : 0;
}

int a3vt_chamfer_fwd_ws(const float *x, const float *y, int draws, int batch, int p, int q, float *dist_xy,
                        int32_t *idx_xy, float *dist_yx, int32_t *idx_yx, float *cd, void *workspace,
                        size_t workspace_bytes, int algo, void *stream) {
  A3VT_CHECK_ARG(x && y && dist_xy && idx_xy && dist_yx && idx_yx && cd);
  ProfScope psc(PROF_SEARCH, static_cast<hipStream_t>(stream));
  return launch_chamfer_fwd(x, y, draws, batch, p, q, dist_xy, idx_xy, dist_yx, idx_yx, cd, workspace,
                            workspace ? workspace_bytes : 0, algo, static_cast<hipStream_t>(stream));
}

int a3vt_chamfer_fwd_shared(const float *x, const float *y, int draws, int batch, int y_batch, int p, int q, float *dist_xy,
                            int32_t *idx_xy, float *dist_yx, int32_t *idx_yx, float *cd, void *workspace,
                            size_t workspace_bytes, int algo, void *stream) {
  A3VT_CHECK_ARG(x && y && dist_xy && idx_xy && dist_yx && idx_yx && cd && y_batch > 0);
  ProfScope psc(PROF_SEARCH, static_cast<hipStream_t>(stream));
  return launch_chamfer_fwd(x, y, draws, batch, p, q, dist_xy, idx_xy, dist_yx, idx_yx, cd, workspace,
                            workspace ? workspace_bytes : 0, algo, static_cast<hipStream_t>(stream), y_batch);
}

int a3vt_chamfer_bwd(const float *x, const float *y, int draws, int batch, int p, int q, const int32_t *idx_xy,
                     const int32_t *idx_yx, const float *grad_cd, float *grad_x, float *grad_y, void *stream) {
  A3VT_CHECK_ARG(x && y && idx_xy && idx_yx && grad_cd && grad_x && draws > 0 && batch > 0 && p > 0 && q > 0);
  ProfScope psc(PROF_LOSS, static_cast<hipStream_t>(stream));
  return launch_chamfer_bwd(x, y, draws, batch, p, q, idx_xy, idx_yx, grad_cd, grad_x, grad_y,
                            static_cast<hipStream_t>(stream));
}

static int fill_pool_args(PoolArgs &a, const float *verts, int batch, int n_vert, const float *proj, int n_maps,
                          const float *const *maps, const int *chans, const int *heights, const int *widths, int ld) {
  A3VT_CHECK_ARG(verts && proj && maps && chans && heights && widths && batch > 0 && n_vert > 0);
  A3VT_CHECK_ARG(n_maps >= 1 && n_maps <= kMaxMaps);
  a.verts = verts;
  for (int i = 0; i < 12; ++i) a.proj[i] = proj[i];
  a.batch = batch;
  a.n_vert = n_vert;
  a.n_maps = n_maps;
  int off = 0;
  for (int k = 0; k < n_maps; ++k) {
    A3VT_CHECK_ARG(maps[k] != nullptr);
    a.maps[k] = maps[k];
    a.C[k] = chans[k];
    a.H[k] = heights[k];
    a.W[k] = widths[k];
    a.off[k] = off;
    off += chans[k];
  }
  a.ld = ld;
  return 0;
}

int a3vt_image_pool_fwd(const float *verts, int batch, int n_vert, const float *proj, int n_maps,
                        const float *const *maps, const int *chans, const int *heights, const int *widths,
                        float *feats, int ld_feats, void *stream) {
  PoolArgs a{};
  if (int rc = fill_pool_args(a, verts, batch, n_vert, proj, n_maps, maps, chans, heights, widths, ld_feats)) return rc;
  A3VT_CHECK_ARG(feats != nullptr);
  a.feats = feats;
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_pool_fwd(a, static_cast<hipStream_t>(stream));
}

int a3vt_image_pool_fwd_add(const float *verts, int batch, int n_vert, const float *proj, int n_maps,
                            const float *const *maps, const int *chans, const int *heights, const int *widths,
                            const float *base, float *feats, int ld_feats, void *stream) {
  PoolArgs a{};
  if (int rc = fill_pool_args(a, verts, batch, n_vert, proj, n_maps, maps, chans, heights, widths, ld_feats)) return rc;
  A3VT_CHECK_ARG(feats != nullptr && base != nullptr);
  int width = 0;
  for (int k = 0; k < n_maps; ++k) width += chans[k];
  A3VT_CHECK_ARG(width == ld_feats);     // every column of a row is written: feats = base + pooled
  a.feats = feats;
  a.base = base;
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_pool_fwd(a, static_cast<hipStream_t>(stream));
}

int a3vt_image_pool_bwd(const float *verts, int batch, int n_vert, const float *proj, int n_maps,
                        const float *const *maps, const int *chans, const int *heights, const int *widths,
                        const float *grad_feats, int ld_feats, float *const *grad_maps, float *grad_verts,
                        void *stream) {
  PoolArgs a{};
  if (int rc = fill_pool_args(a, verts, batch, n_vert, proj, n_maps, maps, chans, heights, widths, ld_feats)) return rc;
  A3VT_CHECK_ARG(grad_feats && grad_maps && grad_verts);
  for (int k = 0; k < n_maps; ++k) {
    A3VT_CHECK_ARG(grad_maps[k] != nullptr);
    a.gmaps[k] = grad_maps[k];
  }
  a.gfeats = grad_feats;
  a.gverts = grad_verts;
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_pool_bwd(a, static_cast<hipStream_t>(stream));
}

size_t a3vt_bias_grad_scratch_bytes(long long rows, int channels) {
  if (rows <= 0 || channels <= 0) return 0;
  return (size_t)bias_grad_wgs(rows * channels, channels) * channels * sizeof(float);
}

int a3vt_bias_grad_nhwc(const void *grad, int bf16, long long rows, int channels, float *out, void *scratch,
                        size_t scratch_bytes, void *stream) {
  A3VT_CHECK_ARG(grad && out && scratch);
  A3VT_CHECK_ARG(rows > 0 && channels > 0 && (bf16 == 0 || bf16 == 1));
  A3VT_CHECK_ARG(aligned_to(grad, 16));
  const size_t need = a3vt_bias_grad_scratch_bytes(rows, channels);
  A3VT_CHECK_ARG(need > 0 && scratch_bytes >= need);
  return launch_bias_grad(grad, bf16, rows, channels, out, static_cast<float *>(scratch), static_cast<hipStream_t>(stream));
}

size_t a3vt_bnrelu_scratch_bytes(int channels) { return channels > 0 ? bnrelu_scratch_bytes(channels) : 0; }

int a3vt_bnrelu_fwd(const void *x, long long rows, int channels, const float *gamma, const float *beta, const float *pre_bias,
                    float eps, float momentum, float *running_mean, float *running_var, long long *num_batches_tracked, void *y,
                    float *save, void *scratch, size_t scratch_bytes, void *stream) {
  A3VT_CHECK_ARG(x && y && gamma && beta && save && scratch);
  A3VT_CHECK_ARG(rows >= 2 && channels > 0 && rows <= (1ll << 40) / channels);
  A3VT_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr));
  A3VT_CHECK_ARG(eps >= 0.f && momentum >= 0.f && momentum <= 1.f);
  A3VT_CHECK_ARG(aligned_to(x, 16) && aligned_to(y, 16) && aligned_to(scratch, 16));
  A3VT_CHECK_ARG(bnrelu_wgs(rows * channels, channels, 4, 1024) > 0 && scratch_bytes >= bnrelu_scratch_bytes(channels));
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_bnrelu_fwd(x, rows, channels, gamma, beta, pre_bias, eps, momentum, running_mean, running_var, num_batches_tracked, y,
                           save, scratch, static_cast<hipStream_t>(stream));
}

int a3vt_bnrelu_bwd(const void *dy, const void *x, long long rows, int channels, const float *save, void *dx, float *dgamma,
                    float *dbeta, float *dx_colsum, void *scratch, size_t scratch_bytes, void *stream) {
  A3VT_CHECK_ARG(dy && x && save && dx && dgamma && dbeta && scratch);
  A3VT_CHECK_ARG(rows >= 2 && channels > 0 && rows <= (1ll << 40) / channels);
  A3VT_CHECK_ARG(aligned_to(x, 16) && aligned_to(dy, 16) && aligned_to(dx, 16) && aligned_to(scratch, 16));
  A3VT_CHECK_ARG(bnrelu_wgs(rows * channels, channels, 4, 1024) > 0 && scratch_bytes >= bnrelu_scratch_bytes(channels));
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_bnrelu_bwd(dy, x, rows, channels, save, dx, dgamma, dbeta, dx_colsum, scratch, static_cast<hipStream_t>(stream));
}

int a3vt_cast_weights_bf16(int n, const float *const *src, void *const *dst, const long long *outer, const int *inner,
                           const int *hw, void *stream) {
  A3VT_CHECK_ARG(n >= 0 && n <= kCastBatchMax);
  A3VT_CHECK_ARG(n == 0 || (src && dst && outer && inner && hw));
  CastBatch b;
  b.n = n;
  b.start[0] = 0;
  for (int k = 0; k < n; ++k) {
    A3VT_CHECK_ARG(src[k] && dst[k] && outer[k] > 0 && inner[k] > 0 && hw[k] > 0);
    A3VT_CHECK_ARG(outer[k] <= (1ll << 31) / inner[k] / hw[k]);
    b.src[k] = src[k];
    b.dst[k] = static_cast<uint16_t *>(dst[k]);
    b.inner[k] = inner[k];
    b.hw[k] = hw[k];
    b.start[k + 1] = b.start[k] + outer[k] * inner[k] * hw[k];
  }
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_cast_weights(b, static_cast<hipStream_t>(stream));
}

int a3vt_conv5_supported(int cin, int cout, int stride) { return conv5_shape_ok(cin, cout, stride) ? 1 : 0; }

size_t a3vt_conv5_image_bytes(int cout, int cin, int flip) {
  if (cin == 3 && flip) return cout == 16 ? conv5_weight_image_bytes(16, 16) : 0;     // (the input gradient of layer 1)
  if (cin == 3) return cout == 3 || cout == 16 ? conv5_weight_image_bytes(cout, 3) : 0;
  if ((cin != 16 && cin != 32) || (cout != 16 && cout != 32)) return 0;
  return flip ? conv5_weight_image_bytes(cin, cout) : conv5_weight_image_bytes(cout, cin);
}

int a3vt_conv5_weight_image(const float *weight, int cout, int cin, int flip, void *image, void *stream) {
  A3VT_CHECK_ARG(weight && image && (flip == 0 || flip == 1));
  A3VT_CHECK_ARG(((cin == 16 || cin == 32) && (cout == 16 || cout == 32)) || (cin == 3 && flip == 0 && (cout == 3 || cout == 16)) ||
                 (cin == 3 && flip == 1 && cout == 16));
  A3VT_CHECK_ARG(aligned_to(image, 16));
  return launch_conv5_weight_image(weight, flip, cout, cin, image, static_cast<hipStream_t>(stream));
}

int a3vt_conv5_nhwc(const void *x, int batch, int height, int width, int cin, int cout, int stride, int pad, const void *image,
                    const float *bias, void *y, void *stream) {
  A3VT_CHECK_ARG(x && image && y);
  A3VT_CHECK_ARG(conv5_shape_ok(cin, cout, stride));
  A3VT_CHECK_ARG(batch > 0 && height > 0 && width > 0 && pad >= 0 && pad <= 4);
  A3VT_CHECK_ARG(height + 2 * pad >= 5 && width + 2 * pad >= 5);
  A3VT_CHECK_ARG((long long)batch * height * width <= (1ll << 31) / 32);
  A3VT_CHECK_ARG(aligned_to(x, cin == 3 ? 2 : 16) && aligned_to(y, cin == 3 ? 2 : 16));
  A3VT_CHECK_ARG(aligned_to(image, 16) && (cout == 3 || aligned_to(y, 16)));
  A3VT_CHECK_ARG(aligned_to(bias, cout == 3 ? 4 : 16));
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_conv5(x, batch, height, width, cin, cout, stride, pad, image, bias, y, static_cast<hipStream_t>(stream));
}

int a3vt_conv5_input_grad_3x16s2(const void *grad_out, int batch, int out_height, int out_width, const void *image, void *grad_in,
                                 void *stream) {
  A3VT_CHECK_ARG(grad_out && image && grad_in && batch > 0 && out_height > 0 && out_width > 0);
  A3VT_CHECK_ARG((long long)batch * (2 * out_height + 2) * (2 * out_width + 2) <= (1ll << 31) / 16);
  A3VT_CHECK_ARG(aligned_to(grad_out, 16) && aligned_to(image, 16));
  A3VT_CHECK_ARG(aligned_to(grad_in, 2));
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_conv5_up3(grad_out, batch, out_height, out_width, image, grad_in, static_cast<hipStream_t>(stream));
}

size_t a3vt_conv5_wrw_scratch_bytes(int cin, int cout) {
  return ((cin == 16 || cin == 32) && (cout == 16 || cout == 32)) || (cin == 3 && (cout == 3 || cout == 16)) ? conv5_wrw_scratch_bytes(cin, cout) : 0;
}

int a3vt_conv5_weight_grad(const void *x, const void *grad_out, int batch, int height, int width, int cin, int cout, int stride,
                           float *grad_weight, void *scratch, size_t scratch_bytes, void *stream) {
  A3VT_CHECK_ARG(x && grad_out && grad_weight && scratch);
  A3VT_CHECK_ARG(conv5_shape_ok(cin, cout, stride));
  A3VT_CHECK_ARG(batch > 0 && height >= 3 && width >= 3 && (long long)batch * height * width <= (1ll << 31) / 32);
  A3VT_CHECK_ARG(aligned_to(scratch, 16));
  A3VT_CHECK_ARG(aligned_to(x, cin == 3 ? 2 : 16) && aligned_to(grad_out, cout == 3 ? 2 : 16));
  A3VT_CHECK_ARG(scratch_bytes >= conv5_wrw_scratch_bytes(cin, cout));
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_conv5_wrw(x, grad_out, batch, height, width, cin, cout, stride, grad_weight, scratch, static_cast<hipStream_t>(stream));
}

int a3vt_conv5f_supported(int cin, int cout, int stride) { return conv5f_shape_ok(cin, cout, stride) ? 1 : 0; }

size_t a3vt_conv5f_image_bytes(int cin, int cout) { return conv5f_weight_image_bytes(cin, cout); }

int a3vt_conv5f_weight_image(const float *weight, int cout, int cin, void *image, void *stream) {
  A3VT_CHECK_ARG(weight && image);
  A3VT_CHECK_ARG(conv5f_weight_image_bytes(cin, cout) != 0);
  A3VT_CHECK_ARG(aligned_to(weight, 4) && aligned_to(image, 16));
  return launch_conv5f_weight_image(weight, cout, cin, image, static_cast<hipStream_t>(stream));
}

int a3vt_conv5f_nhwc(const float *x, int batch, int height, int width, int cin, int cout, int stride, int pad, const void *image,
                     const float *scale, const float *shift, int relu, float *y, void *stream) {
  A3VT_CHECK_ARG(x && image && y);
  A3VT_CHECK_ARG(conv5f_shape_ok(cin, cout, stride));
  A3VT_CHECK_ARG(batch >= 1 && height >= 1 && width >= 1 && pad >= 0 && pad <= 4 && (relu == 0 || relu == 1));
  A3VT_CHECK_ARG(height + 2 * pad >= 5 && width + 2 * pad >= 5);          // (an empty output otherwise)
  A3VT_CHECK_ARG((long long)batch * height * width <= (1ll << 31) / 32);
  A3VT_CHECK_ARG(aligned_to(x, cin == 3 ? 4 : 16));
  A3VT_CHECK_ARG(aligned_to(y, 16) && aligned_to(image, 16));
  A3VT_CHECK_ARG(aligned_to(scale, 4) && aligned_to(shift, 4));
  ProfScope psc(PROF_ENC, static_cast<hipStream_t>(stream));
  return launch_conv5f(x, batch, height, width, cin, cout, stride, pad, image, scale, shift, relu, y, static_cast<hipStream_t>(stream));
}

int a3vt_adam_chunk_elems(void) { return adam_chunk_elems(); }

int a3vt_adam_step(void *const *param, const void *const *grad, void *const *exp_avg, void *const *exp_avg_sq,
                   const long long *numel, const int *chunk_tensor, const long long *chunk_off, int n_chunks, double lr, double beta1,
                   double beta2, double eps, double weight_decay, long long step, void *stream) {
  A3VT_CHECK_ARG(n_chunks >= 0 && step >= 1);
  A3VT_CHECK_ARG(n_chunks == 0 || (param && grad && exp_avg && exp_avg_sq && numel && chunk_tensor && chunk_off));
  A3VT_CHECK_ARG(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0);
  ProfScope psc(PROF_OPT, static_cast<hipStream_t>(stream));
  return launch_adam(param, grad, exp_avg, exp_avg_sq, numel, chunk_tensor, chunk_off, n_chunks, lr, beta1, beta2, eps, weight_decay, step,
                     static_cast<hipStream_t>(stream));
}

int a3vt_adam_step_clamp(void *const *param, void *const *grad, void *const *exp_avg, void *const *exp_avg_sq, const long long *numel,
                         const int *chunk_tensor, const long long *chunk_off, int n_chunks, double lr, double beta1, double beta2,
                         double eps, double weight_decay, long long step, double grad_clamp, void *stream) {
  A3VT_CHECK_ARG(n_chunks >= 0 && step >= 1 && grad_clamp > 0.0);
  A3VT_CHECK_ARG(n_chunks == 0 || (param && grad && exp_avg && exp_avg_sq && numel && chunk_tensor && chunk_off));
  A3VT_CHECK_ARG(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0);
  ProfScope psc(PROF_OPT, static_cast<hipStream_t>(stream));
  return launch_adam(param, const_cast<const void *const *>(grad), exp_avg, exp_avg_sq, numel, chunk_tensor, chunk_off, n_chunks, lr, beta1,
                     beta2, eps, weight_decay, step, static_cast<hipStream_t>(stream), grad_clamp);
}

int a3vt_profile_enable(int on) {
  g_prof.on = on != 0;
  g_prof.used = 0;
  return 0;
}

int a3vt_profile_read_classes(double *total_ms, int *count, int n) {
  A3VT_CHECK_ARG(total_ms && count && n >= 0);
  for (int c = 0; c < n; ++c) { total_ms[c] = 0.0; count[c] = 0; }
  for (int i = 0; i < g_prof.used; ++i) {
    if (hipEventSynchronize(g_prof.ev[i][1]) != hipSuccess) { set_error("profile_read: event sync failed"); return -2; }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_prof.ev[i][0], g_prof.ev[i][1]) != hipSuccess) continue;
    if (g_prof.cls[i] >= n) continue;
    total_ms[g_prof.cls[i]] += ms;
    count[g_prof.cls[i]] += 1;
  }
  g_prof.used = 0;
  return PROF_CLASSES;
}

int a3vt_profile_read(double *total_ms, int *count) {
  const int rc = a3vt_profile_read_classes(total_ms, count, 3);
  return rc < 0 ? rc : 0;
}

int a3vt_dbg_path_counts(long long *counts, int n, int reset) {
  A3VT_CHECK_ARG(n >= 0 && (counts != nullptr || n == 0));
  for (int i = 0; i < n; ++i) counts[i] = i < PATH_COUNT ? g_path_counts[i].load(std::memory_order_relaxed) : 0;
  if (reset)
    for (auto &c : g_path_counts) c.store(0, std::memory_order_relaxed);
  return PATH_COUNT;
}

int a3vt_dbg_csr_algo(int algo) {
  A3VT_CHECK_ARG(algo >= 0 && algo <= 2);
  g_csr_algo = algo;
  return 0;
}

int a3vt_split3_bf16(const float *x, size_t n, uint16_t *hi, uint16_t *mid, uint16_t *lo, void *stream) {
  A3VT_CHECK_ARG(n == 0 || (x && hi && mid && lo));
  return launch_split3(x, n, hi, mid, lo, static_cast<hipStream_t>(stream));
}

int a3vt_check_finite(const float *data, size_t n, int32_t *flag, void *stream) {
  A3VT_CHECK_ARG(data && flag);
  return launch_check_finite(data, n, flag, static_cast<hipStream_t>(stream));
}

}  // extern "C"
