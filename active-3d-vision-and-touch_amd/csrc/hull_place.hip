// hull_place.hip — the hand's placement on the convex hull of a mesh's vertices without building a hull
// (pterotactyl/simulator/physics/grasping.py::place_hand; include/a3vt.h states the rule in full).
//
// place_hand needs one thing of the hull: the farthest point t d of the ray from the origin along an action's direction d that is
// still inside it, and the plane of the facet there.  That is a linear programme in three variables — the largest t with t d in
// the convex hull of the vertices — whose optimal basis is three vertices that span the facet.  It is solved by SUPPORT PASSES:
// the lowest index of the largest n . v_i over the mesh's vertices, for a normal n that the pass before it decides.
//
// ONE workgroup of 256 threads per (mesh, action), a few dozen sequential passes each.
// * The directions and the launch's vertex ranges travel by value in the kernel arguments (the host has checked them).
// * A pass: every thread strides over the mesh's vertices (read from global memory every time: a 10 242-vertex mesh is 120 KB,
//   which the workgroups of its actions share in L2), converts to double, forms (n.x v.x + n.y v.y) + n.z v.z and keeps the
//   largest value with its lowest index, and the smallest value; a 64-lane butterfly per wave, the four waves' results in LDS
//   behind one barrier; thread 0 joins them, advances the rule by one step — all scalar float64 — and publishes the next normal
//   through LDS behind a second barrier.  The very first pass also takes the largest |coordinate| and looks for non-finite ones.
// * Thread 0 alone holds the rule's state (phase, the basis and its projections) in registers and writes the outputs.
// No atomics, no workspace: two calls write the same bytes, and a (mesh, action) row does not depend on the rest of the batch.
// The file is built with -ffp-contract=off: ops.py's float64 NumPy form states the same operations in the same order.
#include "common.h"
#include "kernels.h"
#include "prims.h"

namespace a3vt {

namespace {

constexpr int kHullThreads = 256;
constexpr int kHullWaves = kHullThreads / kWave;
constexpr double kHullFlat = 1e-12;        // a hull thinner than this x the mesh's largest |coordinate| along the facet's normal is flat
constexpr double kHullMinSin2 = 1e-24;     // below it the rotation is the reference's reflection case

struct D2 {
  double x, y;
};
struct D3 {
  double x, y, z;
};

__device__ __forceinline__ double dot3(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross3(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double cross2(D2 p, D2 q) { return p.x * q.y - p.y * q.x; }
__device__ __forceinline__ D2 sub2(D2 p, D2 q) { return {p.x - q.x, p.y - q.y}; }
__device__ __forceinline__ D3 vertex(const float *__restrict__ v, int i) {
  return {(double)v[3 * (long long)i], (double)v[3 * (long long)i + 1], (double)v[3 * (long long)i + 2]};
}

// (value, index) pairs: the larger value wins, the lower index among equal values
__device__ __forceinline__ void take_max(double &val, int &idx, double oval, int oidx) {
  if (oval > val || (oval == val && oidx < idx)) {
    val = oval;
    idx = oidx;
  }
}

__global__ __launch_bounds__(kHullThreads) void hull_place_kernel(const float *__restrict__ verts, const HullBatch batch, int m0, int A,
                                                                  double hand_distance, D3 tip, int32_t *__restrict__ status_out,
                                                                  float *__restrict__ base_pos, float *__restrict__ base_rot,
                                                                  int32_t *__restrict__ simplex_out, double *__restrict__ t_out) {
  __shared__ double s_n[3];                       // the normal of the next pass
  __shared__ int s_go;                            // 0: the rule has ended
  __shared__ double s_hi[kHullWaves], s_lo[kHullWaves], s_abs[kHullWaves];
  __shared__ int s_idx[kHullWaves], s_bad[kHullWaves];

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int local = (int)blockIdx.x / A, action = (int)blockIdx.x % A;
  const long long row = ((long long)m0 + local) * A + action;
  const int v0 = batch.offset[local], nv = batch.offset[local + 1] - v0;
  const float *__restrict__ mesh = verts + 3 * (long long)v0;
  const D3 d = {batch.direction[action][0], batch.direction[action][1], batch.direction[action][2]};

  // ---- thread 0's state ----------------------------------------------------------------------------------------------------
  int phase = 0, passes = 0, status = -1;         // phase: which support the pass in flight answers (0, 1: the opening; 2: GJK; 3: pivot)
  int ia = -1, ib = -1, ic = -1;
  D3 fx = {0, 0, 0}, fy = {0, 0, 0}, N = {0, 0, 0};
  D2 pa = {0, 0}, pb = {0, 0}, pc = {0, 0}, u = {0, 0};
  double t = 0.0, largest = 0.0;

  if (tid == 0) {
    // the frame: e = the axis of d's smallest |component| (the lowest on a tie), x = d x e, y = d x x, both of unit length
    const double ax = fabs(d.x), ay = fabs(d.y), az = fabs(d.z);
    const int k = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
    const D3 e = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    fx = cross3(d, e);
    const double lx = sqrt(dot3(fx, fx));
    fx = {fx.x / lx, fx.y / lx, fx.z / lx};
    fy = cross3(d, fx);
    const double ly = sqrt(dot3(fy, fy));
    fy = {fy.x / ly, fy.y / ly, fy.z / ly};
    s_n[0] = fx.x, s_n[1] = fx.y, s_n[2] = fx.z;
    s_go = nv >= 4;
    if (nv < 4) status = 1;
  }

  for (bool first = true;; first = false) {
    __syncthreads();                              // s_n and s_go are published
    if (!s_go) break;
    // ---- one support pass ----------------------------------------------------------------------------------------------------
    const D3 n = {s_n[0], s_n[1], s_n[2]};
    double hi = -INFINITY, lo = INFINITY, big = 0.0;
    int idx = 0x7fffffff, bad = 0;
    for (int i = tid; i < nv; i += kHullThreads) {
      const D3 v = vertex(mesh, i);
      const double val = dot3(n, v);
      if (val > hi) {
        hi = val;
        idx = i;
      }
      lo = fmin(lo, val);
      if (first) {
        const double m = fmax(fabs(v.x), fmax(fabs(v.y), fabs(v.z)));
        bad |= !(fabs(v.x) <= 3.4028234663852886e38 && fabs(v.y) <= 3.4028234663852886e38 && fabs(v.z) <= 3.4028234663852886e38);
        big = fmax(big, m);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ohi = __shfl_xor(hi, off, kWave);
      const int oidx = __shfl_xor(idx, off, kWave);
      take_max(hi, idx, ohi, oidx);
      lo = fmin(lo, __shfl_xor(lo, off, kWave));
      if (first) {
        big = fmax(big, __shfl_xor(big, off, kWave));
        bad |= __shfl_xor(bad, off, kWave);
      }
    }
    if (lane == 0) {
      s_hi[wave] = hi, s_lo[wave] = lo, s_idx[wave] = idx;
      if (first) s_abs[wave] = big, s_bad[wave] = bad;
    }
    __syncthreads();
    if (tid != 0) continue;

    // ---- thread 0: join the waves, advance the rule by one step ------------------------------------------------------------------
    hi = s_hi[0], lo = s_lo[0], idx = s_idx[0];
#pragma unroll
    for (int w = 1; w < kHullWaves; ++w) {
      take_max(hi, idx, s_hi[w], s_idx[w]);
      lo = fmin(lo, s_lo[w]);
    }
    if (first) {
      bad = 0;
#pragma unroll
      for (int w = 0; w < kHullWaves; ++w) {
        largest = fmax(largest, s_abs[w]);
        bad |= s_bad[w];
      }
      if (bad) status = 1;                        // a non-finite coordinate: place_hand's None
    }
    const int w = idx;
    D2 pw = {0, 0};
    if (status < 0 && (unsigned)w < (unsigned)nv) {
      const D3 vw = vertex(mesh, w);
      pw = {dot3(vw, fx), dot3(vw, fy)};
    } else if (status < 0) {
      status = 2;                                 // (no vertex won: every value was a NaN; not reachable for finite vertices)
    }
    bool ask2 = false;                            // the next pass is along the 2-D direction u
    if (status >= 0) {
    } else if (phase == 0) {                      // support along (1, 0)
      ia = w, pa = pw;
      if (pa.x < 0.0) {
        status = 1;
      } else if (pa.x == 0.0) {
        status = 2;
      } else {
        u = {-pa.x, -pa.y};
        ask2 = true;
        phase = 1;
      }
    } else if (phase == 1 || phase == 2) {
      const double sv = pw.x * u.x + pw.y * u.y;
      if (sv < 0.0) {
        status = 1;                               // u separates the origin from the projection: the ray misses
      } else if (sv == 0.0 || w == ia || (phase == 1 ? false : w == ib)) {
        status = 2;
      } else if (phase == 1) {
        ib = w, pb = pw;
        phase = 2;
      } else {
        ic = w, pc = pw;
        const D2 ac = sub2(pc, pa), bc = sub2(pc, pb);
        const double o_ac = cross2(ac, {-pa.x, -pa.y}), b_ac = cross2(ac, sub2(pb, pa));
        const double o_bc = cross2(bc, {-pb.x, -pb.y}), a_bc = cross2(bc, sub2(pa, pb));
        if (o_ac == 0.0 || o_bc == 0.0 || b_ac == 0.0 || a_bc == 0.0) {
          status = 2;
        } else if ((o_ac > 0.0) != (b_ac > 0.0)) {
          ib = ic, pb = pc;                       // the origin is outside edge a c: b leaves
        } else if ((o_bc > 0.0) != (a_bc > 0.0)) {
          ia = ic, pa = pc;                       // outside edge b c: a leaves
        } else {
          phase = 3;                              // the triangle's projection holds the origin
          passes = 0;
        }
      }
      if (status < 0 && phase == 2) {             // the next edge's normal that faces the origin
        if (passes == kHullGjkPasses) {
          status = 2;
        } else {
          const double ex = pb.x - pa.x, ey = pb.y - pa.y;
          const double orient = ey * pa.x - ex * pa.y;
          if (orient == 0.0 && passes > 0) {
            status = 2;                           // the origin on the edge's line (but on the opening edge: between a and b)
          } else {
            u = orient >= 0.0 ? D2{-ey, ex} : D2{ey, -ex};
            ask2 = true;
            ++passes;
          }
        }
      }
    } else {                                      // phase 3, the answer to a pivot's support
      if (hi <= t || w == ia || w == ib || w == ic) {
        // the basis is optimal: the checks
        if (t <= 0.0)
          status = 1;
        else if (hi - lo <= kHullFlat * largest)
          status = 2;
        else
          status = 0;
      } else {
        const double area = cross2(sub2(pb, pa), sub2(pc, pa));
        if (area == 0.0) {
          status = 2;
        } else {
          const double la = fmax(cross2(pb, pc) / area, 0.0), lb = fmax(cross2(pc, pa) / area, 0.0), lc = fmax(cross2(pa, pb) / area, 0.0);
          const double ma = cross2(sub2(pb, pw), sub2(pc, pw)) / area, mb = cross2(sub2(pc, pw), sub2(pa, pw)) / area,
                       mc = cross2(sub2(pa, pw), sub2(pb, pw)) / area;
          int leave = -1;
          double best = 0.0;
          if (ma > 0.0) leave = 0, best = la / ma;
          if (mb > 0.0 && (leave < 0 || lb / mb < best)) leave = 1, best = lb / mb;
          if (mc > 0.0 && (leave < 0 || lc / mc < best)) leave = 2, best = lc / mc;
          if (leave < 0)
            status = 2;
          else if (leave == 0)
            ia = w, pa = pw;
          else if (leave == 1)
            ib = w, pb = pw;
          else
            ic = w, pc = pw;
        }
      }
    }
    if (status < 0 && phase == 3) {               // the basis's plane, and the pass that tests it
      if (passes == kHullPivotPasses) {
        status = 2;
      } else {
        const D3 a = vertex(mesh, ia), b = vertex(mesh, ib), c = vertex(mesh, ic);
        N = cross3({b.x - a.x, b.y - a.y, b.z - a.z}, {c.x - a.x, c.y - a.y, c.z - a.z});
        const double den = dot3(N, d);
        if (den == 0.0) {
          status = 2;
        } else {
          const D3 nn = {N.x / den, N.y / den, N.z / den};
          t = dot3(nn, a);
          s_n[0] = nn.x, s_n[1] = nn.y, s_n[2] = nn.z;
          ++passes;
        }
      }
    }
    if (ask2) s_n[0] = u.x * fx.x + u.y * fy.x, s_n[1] = u.x * fx.y + u.y * fy.y, s_n[2] = u.x * fx.z + u.y * fy.z;
    if (status >= 0) s_go = 0;
  }

  // ---- the pose (thread 0): place_hand line for line, float64 ----------------------------------------------------------------------
  if (tid != 0) return;
  double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, base[3] = {0, 0, 0};
  if (status == 0) {
    const D3 point = {d.x * t, d.y * t, d.z * t};
    double len = sqrt(dot3(N, N));
    D3 normal = {N.x / len, N.y / len, N.z / len};
    const D3 moved = {point.x + normal.x * 0.0001, point.y + normal.y * 0.0001, point.z + normal.z * 0.0001};
    if (dot3(point, point) > dot3(moved, moved)) normal = {-normal.x, -normal.y, -normal.z};
    const D3 position = {point.x + normal.x * hand_distance, point.y + normal.y * hand_distance, point.z + normal.z * hand_distance};
    normal = {normal.x - 0.001, normal.y - 0.001, normal.z - 0.001};
    len = sqrt(dot3(normal, normal));
    const double bx = normal.x / len, by = normal.y / len, bz = normal.z / len;
    const double cosine = -bx, sin2 = bz * bz + by * by;     // (-1, 0, 0) x b = (0, bz, -by)
    if (sin2 < kHullMinSin2) {
      status = 2;
    } else {
      const double vx = 0.0, vy = bz, vz = -by;
      const double K[9] = {0.0, -vz, vy, vz, 0.0, -vx, -vy, vx, 0.0};
      const double f = (1.0 - cosine) / sin2;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
          R[3 * i + j] = ((i == j ? 1.0 : 0.0) + K[3 * i + j]) + kk * f;
        }
      const double px[3] = {position.x, position.y, position.z};
#pragma unroll
      for (int i = 0; i < 3; ++i) base[i] = px[i] - ((R[3 * i] * tip.x + R[3 * i + 1] * tip.y) + R[3 * i + 2] * tip.z);
    }
  }
  const bool placed = status == 0;
  status_out[row] = status;
  t_out[row] = placed ? t : 0.0;
  simplex_out[3 * row] = placed ? ia : -1, simplex_out[3 * row + 1] = placed ? ib : -1, simplex_out[3 * row + 2] = placed ? ic : -1;
#pragma unroll
  for (int i = 0; i < 3; ++i) base_pos[3 * row + i] = placed ? (float)base[i] : 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) base_rot[9 * row + i] = placed ? (float)R[i] : 0.f;
}

}  // namespace

int launch_hull_place(const float *verts, const int32_t *vert_offset, int M, const double *directions, int A, double hand_distance,
                      const double *tip_offset, int32_t *status, float *base_pos, float *base_rot, int32_t *simplex, double *t,
                      hipStream_t s) {
  HullBatch batch = {};
  for (int a = 0; a < A; ++a)
    for (int i = 0; i < 3; ++i) batch.direction[a][i] = directions[3 * a + i];
  const D3 tip = {tip_offset[0], tip_offset[1], tip_offset[2]};
  int launches = 0;
  for (int m0 = 0; m0 < M; m0 += kHullMeshesPerLaunch) {
    const int n = M - m0 < kHullMeshesPerLaunch ? M - m0 : kHullMeshesPerLaunch;
    for (int i = 0; i <= n; ++i) batch.offset[i] = vert_offset[m0 + i];
    A3VT_LAUNCH(hull_place_kernel, dim3(n * A), dim3(kHullThreads), 0, s, verts, batch, m0, A, hand_distance, tip, status, base_pos, base_rot,
                simplex, t);
    A3VT_CHECK_LAUNCH();
    ++launches;
  }
  return launches;
}

}  // namespace a3vt
