// voxel.hip — the ground-truth point cloud of a mesh (reference: utility/data_making.py::extract_points over utility/utils.py's
// mesh_to_voxel, extract_ODMs, apply_ODMs, voxel_to_pointcloud, realign_points), for a batch of M meshes in a fixed number of
// launches.  The reference subdivides level by level with a host read per level, loops in Python over every occupied voxel and
// every depth-map pixel and fills holes with SciPy on the host.
//
//   voxel_range     one workgroup per mesh: the scalar min / max over every finite coordinate (the normalisation) and the per-axis
//                   min / max (the realignment); it also resets the mesh's surface statistics.
//   voxel_mark      one wave per face.  Lane l takes the sub-triangle of depth 3 whose path is l's three base-4 digits (it re-derives
//                   its three ancestors, a few flops, instead of exchanging them), so a face that needs it is 64 sub-triangles wide
//                   before any lane walks alone; then every lane walks its own subtree depth-first with its stack of parents in LDS.
//                   A sub-triangle stops when its longest squared side is not above (1 / dim)^2, so siblings stop at different
//                   depths.  Every midpoint is marked by the first lane below its triangle: one plain byte store of 1, idempotent,
//                   so neither the order nor the number of writers shows.
//   voxel_columns   one thread per column of each of the three axes: first and last occupied voxel, stored as the reference's six
//                   orthographic depth maps.
//   voxel_carve     one thread per voxel: kept = inside the interval of its column along each axis.  Written over the occupancy.
//                   (This IS apply_ODMs including binary_fill_holes: a carved voxel lies outside its column's interval along some
//                   axis, and so does every voxel beyond it in that column out to the border, so no carved region is enclosed.)
//   voxel_rows      one wave per (i, j) row: surface = kept and fewer than 27 kept voxels in the 3 x 3 x 3 neighbourhood; the row's
//                   count, and the per-axis integer min / max of the surface (integer atomics: exact in any order).
//   voxel_scan      one workgroup per mesh: exclusive scan of the row counts, the mesh's count.
//   voxel_offsets   one thread: the meshes' offsets into the concatenated surface list.
//   voxel_emit      voxel_rows again, now writing (i, j, k) at offset + rank: (i, j, k)-lexicographic, which is torch.where's order.
//   voxel_gather    one thread per output row: the realigned coordinates of surface row index % n.
// Every float operation that the reference's result depends on is spelled with an explicitly rounded intrinsic, and the file is
// compiled with -ffp-contract=off (lib.py::EXTRA_FLAGS): no multiply-add is fused, so the grids equal the reference's bit for bit.
#include <math.h>

#include <mutex>

#include "common.h"
#include "kernels.h"

namespace a3vt {

namespace {

constexpr int kStartDepth = 3;                              // 4^3 = 64 sub-triangles: one per lane
constexpr int kStackLevels = kVoxelMaxDepth - kStartDepth;   // parents a lane can hold: depths 3 .. kVoxelMaxDepth - 1
constexpr int kRowThreads = 256, kScanThreads = 1024;

struct V3 {
  float x, y, z;
};
struct Tri {
  V3 a, b, c;
};

__device__ __forceinline__ V3 mid(V3 p, V3 q) {   // (p + q) / 2.
  return {__fmul_rn(__fadd_rn(p.x, q.x), 0.5f), __fmul_rn(__fadd_rn(p.y, q.y), 0.5f), __fmul_rn(__fadd_rn(p.z, q.z), 0.5f)};
}
__device__ __forceinline__ float side2(V3 p, V3 q) {   // (abs(p - q) ** 2).sum()
  const float dx = __fsub_rn(p.x, q.x), dy = __fsub_rn(p.y, q.y), dz = __fsub_rn(p.z, q.z);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}
__device__ __forceinline__ bool splits(const Tri &t, float thr) {
  return fmaxf(fmaxf(side2(t.a, t.b), side2(t.b, t.c)), side2(t.c, t.a)) > thr;
}
// The reference's four children of (v1, v2, v3) with v4 = (v1 + v3) / 2, v5 = (v1 + v2) / 2, v6 = (v2 + v3) / 2.
__device__ __forceinline__ Tri child(const Tri &t, int q) {
  const V3 v4 = mid(t.a, t.c), v5 = mid(t.a, t.b), v6 = mid(t.b, t.c);
  switch (q) {
    case 0: return {t.a, v4, v5};
    case 1: return {v5, t.b, v6};
    case 2: return {v5, v4, v6};
    default: return {v4, t.c, v6};
  }
}
__device__ __forceinline__ bool finite3(V3 p) { return fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY; }

__device__ __forceinline__ void mark(uint8_t *grid, int dim, V3 p) {   // ((p + .5) * (dim - 1)).long()
  const float s = (float)(dim - 1);
  const float fx = __fmul_rn(__fadd_rn(p.x, 0.5f), s), fy = __fmul_rn(__fadd_rn(p.y, 0.5f), s), fz = __fmul_rn(__fadd_rn(p.z, 0.5f), s);
  const float top = (float)dim;
  if (fx >= 0.f && fx < top && fy >= 0.f && fy < top && fz >= 0.f && fz < top)   // (always, for a finite face; false for a NaN)
    grid[((long long)(int)fx * dim + (int)fy) * dim + (int)fz] = 1;
}
__device__ __forceinline__ void mark_mids(uint8_t *grid, int dim, const Tri &t) {
  mark(grid, dim, mid(t.a, t.c));
  mark(grid, dim, mid(t.a, t.b));
  mark(grid, dim, mid(t.b, t.c));
}

__device__ __forceinline__ bool is_finite(float x) { return fabsf(x) < INFINITY; }   // (false for a NaN)

// range[m]: {min, max over all coordinates, then min, max per axis}; stats[m]: {min i, max i, min j, max j, min k, max k} of the surface
__global__ __launch_bounds__(256) void voxel_range_kernel(const float *__restrict__ verts, int V, const int32_t *__restrict__ vert_offset,
                                                          int dim, float *__restrict__ range, int32_t *__restrict__ stats) {
  __shared__ float red[8][256 / kWave];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int v0 = min(max(vert_offset[m], 0), V), v1 = min(max(vert_offset[m + 1], v0), V);
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int v = v0 + tid; v < v1; v += 256) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = verts[3ll * v + a];
      if (is_finite(x)) lo[a] = fminf(lo[a], x), hi[a] = fmaxf(hi[a], x);
    }
  }
  float val[8] = {fminf(fminf(lo[0], lo[1]), lo[2]), fmaxf(fmaxf(hi[0], hi[1]), hi[2]), lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]};
#pragma unroll
  for (int q = 0; q < 8; ++q) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const float o = __shfl_xor(val[q], off, kWave);
      val[q] = (q & 1) ? fmaxf(val[q], o) : fminf(val[q], o);
    }
    if (lane == 0) red[q][wave] = val[q];
  }
  __syncthreads();
  if (tid < 8) {
    float r = red[tid][0];
    for (int w = 1; w < 256 / kWave; ++w) r = (tid & 1) ? fmaxf(r, red[tid][w]) : fminf(r, red[tid][w]);
    range[8 * m + tid] = r;
  }
  if (tid < 6) stats[6 * m + tid] = (tid & 1) ? -1 : dim;
}

__global__ __launch_bounds__(kWave) void voxel_mark_kernel(const float *__restrict__ verts, int V, const int32_t *__restrict__ faces, int F,
                                                           const int32_t *__restrict__ vert_offset, const int32_t *__restrict__ face_offset,
                                                           int M, int dim, float thr, const float *__restrict__ range,
                                                           uint8_t *__restrict__ grids) {
  __shared__ float stack[kStackLevels][9][kWave];
  const int lane = threadIdx.x, f = blockIdx.x;
  // the mesh of face f: the last m with face_offset[m] <= f (offsets clamped into [0, F]; an end below its start is an empty mesh)
  int lo = 0, hi = M;   // invariant: start(lo) <= f, answer in [lo, hi)
  while (hi - lo > 1) {
    const int c = (lo + hi) >> 1;
    if (min(max(face_offset[c], 0), F) <= f) lo = c; else hi = c;
  }
  const int m = lo;
  const int f0 = min(max(face_offset[m], 0), F), f1 = min(max(face_offset[m + 1], f0), F);
  if (f < f0 || f >= f1) return;   // (uniform) a face no mesh owns
  const int v0 = min(max(vert_offset[m], 0), V), v1 = min(max(vert_offset[m + 1], v0), V), nv = v1 - v0;
  const int i0 = faces[3ll * f], i1 = faces[3ll * f + 1], i2 = faces[3ll * f + 2];
  if ((unsigned)i0 >= (unsigned)nv || (unsigned)i1 >= (unsigned)nv || (unsigned)i2 >= (unsigned)nv) return;   // (uniform)
  const float vmin = range[8 * m], den = __fsub_rn(range[8 * m + 1], vmin);
  auto load = [&](int i) {   // (v - min) / (max - min) - 0.5
    const float *p = verts + 3ll * (v0 + i);
    return V3{__fsub_rn(__fdiv_rn(__fsub_rn(p[0], vmin), den), 0.5f), __fsub_rn(__fdiv_rn(__fsub_rn(p[1], vmin), den), 0.5f),
              __fsub_rn(__fdiv_rn(__fsub_rn(p[2], vmin), den), 0.5f)};
  };
  Tri cur = {load(i0), load(i1), load(i2)};
  if (!finite3(cur.a) || !finite3(cur.b) || !finite3(cur.c)) return;   // (uniform) non-finite coordinates mark nothing
  uint8_t *grid = grids + (long long)m * dim * dim * dim;
  if (lane == 0) mark(grid, dim, cur.a), mark(grid, dim, cur.b), mark(grid, dim, cur.c);

  // down to this lane's sub-triangle of depth 3; the first lane below a triangle marks its midpoints
#pragma unroll
  for (int level = 0; level < kStartDepth; ++level) {
    if (!splits(cur, thr)) return;
    if ((lane >> (2 * level)) == 0) mark_mids(grid, dim, cur);
    cur = child(cur, (lane >> (2 * level)) & 3);
  }

  // depth-first below it: stack[l] is the parent at depth 3 + l, `path` holds the child being visited of each (2 bits a level)
  int sp = 0;
  unsigned path = 0;
  for (;;) {
    if (sp < kStackLevels && splits(cur, thr)) {
      mark_mids(grid, dim, cur);
      stack[sp][0][lane] = cur.a.x, stack[sp][1][lane] = cur.a.y, stack[sp][2][lane] = cur.a.z;
      stack[sp][3][lane] = cur.b.x, stack[sp][4][lane] = cur.b.y, stack[sp][5][lane] = cur.b.z;
      stack[sp][6][lane] = cur.c.x, stack[sp][7][lane] = cur.c.y, stack[sp][8][lane] = cur.c.z;
      path &= ~(3u << (2 * sp));
      ++sp;
      cur = child(cur, 0);
      continue;
    }
    bool next = false;
    while (sp > 0) {
      const unsigned q = (path >> (2 * (sp - 1))) & 3u;
      if (q < 3u) {
        path += 1u << (2 * (sp - 1));
        const int l = sp - 1;
        const Tri parent = {{stack[l][0][lane], stack[l][1][lane], stack[l][2][lane]},
                            {stack[l][3][lane], stack[l][4][lane], stack[l][5][lane]},
                            {stack[l][6][lane], stack[l][7][lane], stack[l][8][lane]}};
        cur = child(parent, (int)q + 1);
        next = true;
        break;
      }
      --sp;
    }
    if (!next) return;
  }
}

// odm[m][6][dim][dim]: [0] dim - 1 - last k of column (i, j), [1] its first k; [2], [3] the same along j for (i, k); [4], [5] along i
// for (j, k); dim where the column is empty.
__global__ __launch_bounds__(256) void voxel_columns_kernel(const uint8_t *__restrict__ grids, int M, int dim, int32_t *__restrict__ odm) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x, cols = (long long)dim * dim;
  if (t >= 3 * cols * M) return;
  const int m = (int)(t / (3 * cols)), axis = (int)(t / cols % 3), p = (int)(t % cols / dim), q = (int)(t % dim);
  const uint8_t *g = grids + (long long)m * dim * cols;
  long long base, step;
  if (axis == 0) base = (long long)p * cols + (long long)q * dim, step = 1;
  else if (axis == 1) base = (long long)p * cols + q, step = dim;
  else base = (long long)p * dim + q, step = cols;
  int first = dim, last = -1;
  for (int x = 0; x < dim; ++x)
    if (g[base + x * step] != 0) {
      first = min(first, x);
      last = x;
    }
  int32_t *o = odm + ((long long)m * 6 + 2 * axis) * cols + (long long)p * dim + q;
  o[0] = last >= 0 ? dim - 1 - last : dim;
  o[cols] = first;
}

__global__ __launch_bounds__(256) void voxel_carve_kernel(const int32_t *__restrict__ odm, int M, int dim, uint8_t *__restrict__ grids) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x, cols = (long long)dim * dim, cells = cols * dim;
  if (t >= cells * M) return;
  const int m = (int)(t / cells), i = (int)(t % cells / cols), j = (int)(t % cols / dim), k = (int)(t % dim);
  const int32_t *o = odm + (long long)m * 6 * cols;
  const long long ij = (long long)i * dim + j, ik = (long long)i * dim + k, jk = (long long)j * dim + k;
  const bool kept = k >= o[cols + ij] && k <= dim - 1 - o[ij] && j >= o[3 * cols + ik] && j <= dim - 1 - o[2 * cols + ik] &&
                    i >= o[5 * cols + jk] && i <= dim - 1 - o[4 * cols + jk];
  grids[t] = kept ? 1 : 0;
}

// Whether voxel (i, j, k) of the kept grid g is on the surface.  Out-of-grid neighbours count as empty.
__device__ __forceinline__ bool on_surface(const uint8_t *g, int dim, int i, int j, int k) {
  if (k >= dim || g[((long long)i * dim + j) * dim + k] == 0) return false;
  int n = 0;
  for (int di = -1; di <= 1; ++di) {
    const int a = i + di;
    if (a < 0 || a >= dim) continue;
    for (int dj = -1; dj <= 1; ++dj) {
      const int b = j + dj;
      if (b < 0 || b >= dim) continue;
      const uint8_t *row = g + ((long long)a * dim + b) * dim;
      n += (k > 0 ? row[k - 1] : 0) + row[k] + (k + 1 < dim ? row[k + 1] : 0);
    }
  }
  return n < 27;
}

// One wave per (m, i, j) row.  EMIT = false: the row's surface count and the surface's integer bounds.  EMIT = true: the coordinates.
template <bool EMIT>
__global__ __launch_bounds__(kRowThreads) void voxel_rows_kernel(const uint8_t *__restrict__ grids, int M, int dim,
                                                                 int32_t *__restrict__ rowcount, int32_t *__restrict__ stats,
                                                                 const int32_t *__restrict__ rowoff, const int32_t *__restrict__ meshoff,
                                                                 long long total, int32_t *__restrict__ surface) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long row = (long long)blockIdx.x * (kRowThreads / kWave) + threadIdx.x / kWave, cols = (long long)dim * dim;
  if (row >= cols * M) return;   // (wave-uniform)
  const int m = (int)(row / cols), i = (int)(row % cols / dim), j = (int)(row % dim);
  const uint8_t *g = grids + (long long)m * cols * dim;
  int count = 0, kmin = dim, kmax = -1;
  long long at = EMIT ? (long long)meshoff[m] + rowoff[row] : 0;
  for (int k0 = 0; k0 < dim; k0 += kWave) {
    const bool s = on_surface(g, dim, i, j, k0 + lane);
    const unsigned long long vote = __ballot(s);
    if (EMIT) {
      const long long pos = at + __popcll(vote & ((1ull << lane) - 1ull));
      if (s && pos < total) surface[3 * pos] = i, surface[3 * pos + 1] = j, surface[3 * pos + 2] = k0 + lane;
      at += __popcll(vote);
    } else if (vote) {
      count += __popcll(vote);
      kmin = min(kmin, k0 + __ffsll((long long)vote) - 1);
      kmax = max(kmax, k0 + 63 - __clzll((long long)vote));
    }
  }
  if (!EMIT && lane == 0) {
    rowcount[row] = count;
    if (count) {
      int32_t *st = stats + 6 * m;
      atomicMin(st + 0, i), atomicMax(st + 1, i), atomicMin(st + 2, j), atomicMax(st + 3, j), atomicMin(st + 4, kmin), atomicMax(st + 5, kmax);
    }
  }
}

// In place: rows[m][r] becomes the number of surface voxels in the rows before r of mesh m; counts[m] their total.
__global__ __launch_bounds__(kScanThreads) void voxel_scan_kernel(int32_t *__restrict__ rows, int dim, int32_t *__restrict__ counts,
                                                                  int32_t *__restrict__ counts_out) {
  __shared__ int wave_sum[kScanThreads / kWave];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int n = dim * dim, per = (n + kScanThreads - 1) / kScanThreads;
  int32_t *r = rows + (long long)m * n;
  const int b = min(tid * per, n), e = min(b + per, n);
  int sum = 0;
  for (int x = b; x < e; ++x) sum += r[x];
  int scan = sum;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int up = __shfl_up(scan, off, kWave);
    if (lane >= off) scan += up;
  }
  if (lane == kWave - 1) wave_sum[wave] = scan;
  __syncthreads();
  int first = scan - sum, total = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / kWave; ++w) {
    if (w < wave) first += wave_sum[w];
    total += wave_sum[w];
  }
  for (int x = b; x < e; ++x) {
    const int c = r[x];
    r[x] = first;
    first += c;
  }
  if (tid == 0) {
    counts[m] = total;
    if (counts_out) counts_out[m] = total;
  }
}

__global__ void voxel_offsets_kernel(const int32_t *__restrict__ counts, int M, int32_t *__restrict__ meshoff) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  long long at = 0;
  for (int m = 0; m < M; ++m) {
    meshoff[m] = (int32_t)min(at, 0x7fffffffll);
    at += counts[m];
  }
  meshoff[M] = (int32_t)min(at, 0x7fffffffll);
}

// realign_points, one axis: centre on (max + min) / 2, the range max + 1 - min of the CENTRED values, times the vertex range, divided.
__device__ __forceinline__ float realign(int x, int lo, int hi, float vlo, float vhi) {
  const float mid = __fmul_rn(__fadd_rn((float)hi, (float)lo), 0.5f);
  const float c = __fsub_rn((float)x, mid), cmax = __fsub_rn((float)hi, mid), cmin = __fsub_rn((float)lo, mid);
  const float p_range = __fsub_rn(__fadd_rn(cmax, 1.f), cmin), v_range = __fsub_rn(vhi, vlo);
  return __fdiv_rn(__fmul_rn(c, v_range), p_range);
}

// rows of `aligned` (all surface rows, when given) and of `cloud` (index[m][p] % n of mesh m's)
__global__ __launch_bounds__(256) void voxel_gather_kernel(const int32_t *__restrict__ surface, const int32_t *__restrict__ meshoff,
                                                           const int32_t *__restrict__ stats, const float *__restrict__ range, int M,
                                                           long long total, float *__restrict__ aligned,
                                                           const long long *__restrict__ index, int num_points, float *__restrict__ cloud) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n_aligned = aligned ? total : 0, n_cloud = cloud ? (long long)M * num_points : 0;
  if (t >= n_aligned + n_cloud) return;
  int m;
  long long src;
  float *out;
  if (t < n_aligned) {
    int lo = 0, hi = M;
    while (hi - lo > 1) {
      const int c = (lo + hi) >> 1;
      if (meshoff[c] <= t) lo = c; else hi = c;
    }
    m = lo, src = t, out = aligned + 3 * t;
  } else {
    const long long u = t - n_aligned;
    m = (int)(u / num_points);
    out = cloud + 3 * u;
    const long long n = (long long)meshoff[m + 1] - meshoff[m];
    if (n <= 0) {   // an empty surface: the rows are zeros
      out[0] = out[1] = out[2] = 0.f;
      return;
    }
    src = meshoff[m] + ((index[u] % n) + n) % n;
  }
  if (src >= total) return;   // (a `total` below the surface's size: nothing to read)
  const int32_t *st = stats + 6 * m;
  const float *vr = range + 8 * m + 2;
#pragma unroll
  for (int a = 0; a < 3; ++a) out[a] = realign(surface[3 * src + a], st[2 * a], st[2 * a + 1], vr[2 * a], vr[2 * a + 1]);
}

// ---- the library's workspace: one per device, grown on demand, cleared per call ------------------------------------------------------
struct VoxelWorkspace {
  char *base = nullptr;
  size_t bytes = 0;
  int M = 0, dim = 0;   // of the a3vt_voxel_surface call whose tables it holds (0: none)
};
VoxelWorkspace g_ws[64];
std::mutex g_ws_mu;

struct VoxelLayout {
  size_t grid, odm, rows, counts, meshoff, range, stats, bytes;
  VoxelLayout(int M, int dim) {
    const size_t cols = (size_t)dim * dim, a = 256;
    size_t at = 0;
    auto take = [&](size_t n) {
      const size_t o = at;
      at = (at + n + a - 1) / a * a;
      return o;
    };
    grid = take((size_t)M * cols * dim);
    odm = take((size_t)M * 6 * cols * 4);
    rows = take((size_t)M * cols * 4);
    counts = take((size_t)M * 4);
    meshoff = take((size_t)(M + 1) * 4);
    range = take((size_t)M * 8 * 4);
    stats = take((size_t)M * 6 * 4);
    bytes = at;
  }
};

VoxelWorkspace *workspace_for(size_t bytes) {   // (g_ws_mu held) the current device's, at least `bytes` large; nullptr: message set
  int dev = 0;
  (void)hipGetDevice(&dev);
  VoxelWorkspace *w = &g_ws[dev & 63];
  if (w->bytes < bytes) {
    if (w->base) (void)hipFree(w->base);
    w->base = nullptr, w->bytes = 0, w->M = w->dim = 0;
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      set_error("voxel: the workspace of %zu bytes could not be allocated", bytes);
      return nullptr;
    }
    w->base = static_cast<char *>(p), w->bytes = bytes;
  }
  return w;
}

}  // namespace

int launch_voxel_depth_maps(const uint8_t *grids, int M, int dim, int32_t *odm, hipStream_t s) {
  const long long n = 3ll * dim * dim * M;
  A3VT_LAUNCH(voxel_columns_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, grids, M, dim, odm);
  A3VT_CHECK_LAUNCH();
  return 1;
}

int launch_voxel_surface(const float *verts, int V, const int32_t *faces, int F, const int32_t *vert_offset, const int32_t *face_offset, int M,
                         int dim, uint8_t *occupancy, int32_t *odm_out, int32_t *counts, hipStream_t s) {
  std::lock_guard<std::mutex> lock(g_ws_mu);
  const VoxelLayout L(M, dim);
  VoxelWorkspace *w = workspace_for(L.bytes);
  if (!w) return -3;
  w->M = w->dim = 0;
  uint8_t *grid = reinterpret_cast<uint8_t *>(w->base + L.grid);
  int32_t *odm = reinterpret_cast<int32_t *>(w->base + L.odm), *rows = reinterpret_cast<int32_t *>(w->base + L.rows);
  int32_t *cnt = reinterpret_cast<int32_t *>(w->base + L.counts), *meshoff = reinterpret_cast<int32_t *>(w->base + L.meshoff);
  int32_t *stats = reinterpret_cast<int32_t *>(w->base + L.stats);
  float *range = reinterpret_cast<float *>(w->base + L.range);
  const long long cols = (long long)dim * dim, cells = cols * dim;
  const float thr = (float)pow(1.0 / (double)dim, 2.0);
  int launches = 0;
  (void)hipGetLastError();
  if (hipMemsetAsync(grid, 0, (size_t)(cells * M), s) != hipSuccess) {
    set_error("voxel_surface: clearing the grids failed");
    return -2;
  }
  ++launches;
  A3VT_LAUNCH(voxel_range_kernel, dim3((unsigned)M), dim3(256), 0, s, verts, V, vert_offset, dim, range, stats);
  A3VT_CHECK_LAUNCH();
  ++launches;
  if (F > 0) {
    A3VT_LAUNCH(voxel_mark_kernel, dim3((unsigned)F), dim3(kWave), 0, s, verts, V, faces, F, vert_offset, face_offset, M, dim, thr, range,
                grid);
    A3VT_CHECK_LAUNCH();
    ++launches;
  }
  if (occupancy) {
    if (hipMemcpyAsync(occupancy, grid, (size_t)(cells * M), hipMemcpyDeviceToDevice, s) != hipSuccess) {
      set_error("voxel_surface: copying the occupancy out failed");
      return -2;
    }
    ++launches;
  }
  if (launch_voxel_depth_maps(grid, M, dim, odm, s) < 0) return -2;
  ++launches;
  if (odm_out) {
    if (hipMemcpyAsync(odm_out, odm, (size_t)(6 * cols * M) * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      set_error("voxel_surface: copying the depth maps out failed");
      return -2;
    }
    ++launches;
  }
  A3VT_LAUNCH(voxel_carve_kernel, dim3((unsigned)cdiv(cells * M, 256)), dim3(256), 0, s, odm, M, dim, grid);
  A3VT_CHECK_LAUNCH();
  A3VT_LAUNCH(voxel_rows_kernel<false>, dim3((unsigned)cdiv(cols * M, kRowThreads / kWave)), dim3(kRowThreads), 0, s, grid, M, dim, rows, stats,
              nullptr, nullptr, 0ll, nullptr);
  A3VT_CHECK_LAUNCH();
  A3VT_LAUNCH(voxel_scan_kernel, dim3((unsigned)M), dim3(kScanThreads), 0, s, rows, dim, cnt, counts);
  A3VT_CHECK_LAUNCH();
  A3VT_LAUNCH(voxel_offsets_kernel, dim3(1), dim3(1), 0, s, cnt, M, meshoff);
  A3VT_CHECK_LAUNCH();
  launches += 4;
  w->M = M, w->dim = dim;
  return launches;
}

int launch_voxel_points(int M, int dim, long long total, int32_t *surface, float *aligned, const long long *index, int num_points,
                        float *cloud, hipStream_t s) {
  std::lock_guard<std::mutex> lock(g_ws_mu);
  int dev = 0;
  (void)hipGetDevice(&dev);
  const VoxelWorkspace *w = &g_ws[dev & 63];
  if (w->M != M || w->dim != dim || !w->base) {
    set_error("voxel_points: M=%d dim=%d, but the workspace holds the tables of an a3vt_voxel_surface call with M=%d dim=%d", M, dim, w->M,
              w->dim);
    return -1;
  }
  const VoxelLayout L(M, dim);
  const uint8_t *grid = reinterpret_cast<const uint8_t *>(w->base + L.grid);
  const int32_t *rows = reinterpret_cast<const int32_t *>(w->base + L.rows), *meshoff = reinterpret_cast<const int32_t *>(w->base + L.meshoff);
  const int32_t *stats = reinterpret_cast<const int32_t *>(w->base + L.stats);
  const float *range = reinterpret_cast<const float *>(w->base + L.range);
  const long long cols = (long long)dim * dim;
  int launches = 0;
  if (total > 0) {
    A3VT_LAUNCH(voxel_rows_kernel<true>, dim3((unsigned)cdiv(cols * M, kRowThreads / kWave)), dim3(kRowThreads), 0, s, grid, M, dim, nullptr,
                nullptr, rows, meshoff, total, surface);
    A3VT_CHECK_LAUNCH();
    ++launches;
  }
  const long long n = (aligned ? total : 0) + (cloud ? (long long)M * num_points : 0);
  if (n > 0) {
    A3VT_LAUNCH(voxel_gather_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, surface, meshoff, stats, range, M, total, aligned, index,
                num_points, cloud);
    A3VT_CHECK_LAUNCH();
    ++launches;
  }
  return launches;
}

}  // namespace a3vt
