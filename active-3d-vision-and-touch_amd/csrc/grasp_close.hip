// grasp_close.hip — the finger closing of the kinematic grasp (pterotactyl/simulator/physics/grasping.py): from a placed hand and the
// object's triangles to the joint angles at which each finger stops, the links' poses and the finger frames.
//
// THE CLOSING RULE IS A KINEMATIC STAND-IN for the reference's five stepSimulation calls under position control.  It is not
// pybullet, and no frame of it has been compared with one of pybullet's.  The rule (include/a3vt.h states it in full): per finger
// chain, for step = 1..S and the chain's four revolute joints from proximal to distal, joint j tries the angle of `step` steps
// towards its upper limit; the try is accepted iff no collision box of link j or of a link distal to it overlaps a triangle of the
// grasp's mesh (13-axis separating-axis test, touching counts as overlap); otherwise the joint is frozen for good.
//
// ONE workgroup per (grasp, finger), 4 * S sequential queries each.
// * The hand table travels by value in the kernel arguments (the host has checked it); so do the face ranges of the launch's
//   grasps, kGraspPerLaunch per launch.
// * Cull, once: the chain's first joint does not move with the angles, and no point of any box of the chain is further from it
//   than `reach` (the host sums the table's joint offsets and box extents).  A triangle whose bounding sphere misses that sphere
//   (plus kGraspSlack) can never overlap a box.  Survivors are compacted as vertex triples into LDS in face order: per chunk of
//   kGraspThreads faces a ballot and mbcnt give the lane's slot, one LDS word per wave the waves' offsets.  The chunk that would not
//   fit, and every face after it, stay in global memory: each query walks them again and applies the same cull test first.  Both
//   walks call the same test on the same float32 values, and the file is built with -ffp-contract=off, so they give the same
//   booleans.
// * A query: thread 0 forms the tentative poses of the links from the tried joint outwards (their parents' accepted poses are in
//   LDS) and the frames of their boxes; barrier; the lanes stride over the candidates, each against every box, leaving at its
//   first hit; ballot per wave, one LDS word per wave; barrier; every thread ORs the waves' words.  No atomics anywhere: the
//   result cannot depend on the order of arrival, and two calls give the same bytes.
// * After the sweep the workgroup writes its 4 angles, 4 step counts, the chain's 7 link poses and the finger frame (the chain's
//   last link).  The accepted poses in LDS are those of the final angles: each was formed from its parent's accepted pose.
//
// Angles: after k steps joint j stands at q0 + k * delta, delta = (upper - q0) / S formed in double on the host, and at `upper`
// exactly for k = S: one multiply and one add in float32.
// A face with a vertex index outside [0, V) is skipped (checked on the device, as touch_render.hip does); a triangle with a
// non-finite coordinate fails the cull's comparison and is skipped too.
#include "common.h"
#include "kernels.h"
#include "prims.h"

namespace a3vt {

namespace {

// The candidate list allows one workgroup per CU, so the workgroup is the CU's whole complement of waves: 16 (measured against 4:
// DESIGN.md).  launch_bounds holds the kernel to 128 VGPRs for that; it needs no scratch.
constexpr int kGraspThreads = 1024;
constexpr int kGraspWaves = kGraspThreads / kWave;
constexpr float kGraspSlack = 1e-4f;       // metres added to the cull's radius: 1000 x the float32 error of the distances compared
constexpr float kGraspMinAxis2 = 1e-24f;   // a cross-product axis with a squared length below this is skipped

struct Vec3 {
  float x, y, z;
};

__device__ __forceinline__ Vec3 load3(const float *p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ float min3(float a, float b, float c) { return fminf(a, fminf(b, c)); }
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(a, fmaxf(b, c)); }

// One projection axis `a` (box frame) against the triangle p0 p1 p2 (box frame) and the box's half-extents: true when it separates.
__device__ __forceinline__ bool separates(Vec3 a, Vec3 p0, Vec3 p1, Vec3 p2, Vec3 h) {
  if (a.x * a.x + a.y * a.y + a.z * a.z < kGraspMinAxis2) return false;
  const float d0 = a.x * p0.x + a.y * p0.y + a.z * p0.z;
  const float d1 = a.x * p1.x + a.y * p1.y + a.z * p1.z;
  const float d2 = a.x * p2.x + a.y * p2.y + a.z * p2.z;
  const float r = h.x * fabsf(a.x) + h.y * fabsf(a.y) + h.z * fabsf(a.z);
  return min3(d0, d1, d2) > r || max3(d0, d1, d2) < -r;
}

// The 13-axis test of the box (centre c, axes = the columns of the row-major r, half-extents h; 15 floats at `box`) against the
// triangle v0 v1 v2.  Touching counts as overlap: an axis separates only with a strict gap.
__device__ __forceinline__ bool box_overlaps(const float *box, Vec3 v0, Vec3 v1, Vec3 v2) {
  const Vec3 c = load3(box), h = load3(box + 12);
  const float *r = box + 3;
  Vec3 p[3];
  const Vec3 v[3] = {v0, v1, v2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float dx = v[k].x - c.x, dy = v[k].y - c.y, dz = v[k].z - c.z;
    p[k] = {r[0] * dx + r[3] * dy + r[6] * dz, r[1] * dx + r[4] * dy + r[7] * dz, r[2] * dx + r[5] * dy + r[8] * dz};
  }
  if (min3(p[0].x, p[1].x, p[2].x) > h.x || max3(p[0].x, p[1].x, p[2].x) < -h.x) return false;
  if (min3(p[0].y, p[1].y, p[2].y) > h.y || max3(p[0].y, p[1].y, p[2].y) < -h.y) return false;
  if (min3(p[0].z, p[1].z, p[2].z) > h.z || max3(p[0].z, p[1].z, p[2].z) < -h.z) return false;
  const Vec3 e[3] = {{p[1].x - p[0].x, p[1].y - p[0].y, p[1].z - p[0].z},
                     {p[2].x - p[1].x, p[2].y - p[1].y, p[2].z - p[1].z},
                     {p[0].x - p[2].x, p[0].y - p[2].y, p[0].z - p[2].z}};
  const Vec3 n = {e[0].y * e[1].z - e[0].z * e[1].y, e[0].z * e[1].x - e[0].x * e[1].z, e[0].x * e[1].y - e[0].y * e[1].x};
  if (separates(n, p[0], p[1], p[2], h)) return false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (separates({0.f, -e[j].z, e[j].y}, p[0], p[1], p[2], h)) return false;   // x axis of the box  x  edge j
    if (separates({e[j].z, 0.f, -e[j].x}, p[0], p[1], p[2], h)) return false;   // y axis
    if (separates({-e[j].y, e[j].x, 0.f}, p[0], p[1], p[2], h)) return false;   // z axis
  }
  return true;
}

__device__ __forceinline__ bool any_box_overlaps(const float *boxes, int nb, Vec3 v0, Vec3 v1, Vec3 v2) {
  for (int b = 0; b < nb; ++b)
    if (box_overlaps(boxes + b * 15, v0, v1, v2)) return true;
  return false;
}

// The cull: the triangle's bounding sphere (about its centroid) against the reach sphere (centre c, radius reach + slack).
__device__ __forceinline__ bool in_reach(Vec3 v0, Vec3 v1, Vec3 v2, Vec3 c, float radius) {
  const Vec3 m = {(v0.x + v1.x + v2.x) * (1.f / 3.f), (v0.y + v1.y + v2.y) * (1.f / 3.f), (v0.z + v1.z + v2.z) * (1.f / 3.f)};
  auto dist2 = [](Vec3 a, Vec3 b) { return (a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y) + (a.z - b.z) * (a.z - b.z); };
  const float rt = sqrtf(max3(dist2(v0, m), dist2(v1, m), dist2(v2, m)));
  return sqrtf(dist2(m, c)) <= radius + rt;   // (false for a non-finite coordinate)
}

// Face f's vertices; false when an index is outside [0, V).
__device__ __forceinline__ bool load_face(const float *__restrict__ verts, int V, const int32_t *__restrict__ faces, int f, Vec3 &v0,
                                          Vec3 &v1, Vec3 &v2) {
  const int i0 = faces[3 * (long long)f], i1 = faces[3 * (long long)f + 1], i2 = faces[3 * (long long)f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
  v0 = load3(verts + 3 * (long long)i0);
  v1 = load3(verts + 3 * (long long)i1);
  v2 = load3(verts + 3 * (long long)i2);
  return true;
}

// out = a * b (3 x 3, row-major)
__device__ __forceinline__ void mat_mul(const float *a, const float *b, float *out) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// The pose of one link from its parent's: R = Rp Ro Rot(axis, angle), p = pp + Rp xyz.
__device__ __forceinline__ void link_pose(const GraspLink &L, const float *Rp, const float *pp, float angle, float *R, float *p) {
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = pp[i] + (Rp[3 * i] * L.xyz[0] + Rp[3 * i + 1] * L.xyz[1] + Rp[3 * i + 2] * L.xyz[2]);
  float fixed[9];
  mat_mul(Rp, L.rot, fixed);
  if (!L.revolute) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = fixed[i];
    return;
  }
  float s, c;
  sincosf(angle, &s, &c);
  const float x = L.axis[0], y = L.axis[1], z = L.axis[2], t = 1.f - c;
  const float turn[9] = {t * x * x + c,     t * x * y - s * z, t * x * z + s * y,   //
                         t * x * y + s * z, t * y * y + c,     t * y * z - s * x,   //
                         t * x * z - s * y, t * y * z + s * x, t * z * z + c};
  mat_mul(fixed, turn, R);
}

__global__ __launch_bounds__(kGraspThreads) void grasp_close_kernel(const float *__restrict__ verts, int V, const int32_t *__restrict__ faces,
                                                                    const GraspRanges ranges, const float *__restrict__ base_pos,
                                                                    const float *__restrict__ base_rot, int g0, const GraspHand hand,
                                                                    int steps, float *__restrict__ q_out, int32_t *__restrict__ blocked_out,
                                                                    float *__restrict__ link_pos, float *__restrict__ link_rot,
                                                                    float *__restrict__ frame_pos, float *__restrict__ frame_rot) {
  __shared__ float s_tri[kGraspCapacity * 9];
  __shared__ float s_R[kGraspChain][9], s_p[kGraspChain][3];      // the accepted poses of the chain's links
  __shared__ float s_TR[kGraspChain][9], s_Tp[kGraspChain][3];    // the tentative ones of a query
  __shared__ float s_box[kGraspChain * 15];
  __shared__ float s_base[12];
  __shared__ int s_nb, s_hit[kGraspWaves], s_cnt[kGraspWaves], s_final[2 * kGraspJoints];

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int local = (int)blockIdx.x / kGraspFingers, finger = (int)blockIdx.x % kGraspFingers;
  const long long g = (long long)g0 + local;
  const int f0 = ranges.f0[local], f1 = ranges.f1[local];
  const GraspLink *chain = hand.link + finger * kGraspChain;

  // ---- the rest pose (thread 0) ------------------------------------------------------------------------------------------------
  if (tid == 0) {
    for (int i = 0; i < 3; ++i) s_base[i] = base_pos[3 * g + i];
    for (int i = 0; i < 9; ++i) s_base[3 + i] = base_rot[9 * g + i];
    for (int k = 0; k < kGraspChain; ++k) {
      const int parent = chain[k].parent;
      link_pose(chain[k], parent < 0 ? s_base + 3 : s_R[parent], parent < 0 ? s_base : s_p[parent], chain[k].q0, s_R[k], s_p[k]);
    }
  }
  __syncthreads();

  // ---- cull and compact --------------------------------------------------------------------------------------------------------
  const Vec3 centre = load3(s_p[0]);
  const float radius = hand.reach[finger] + kGraspSlack;
  int n_lds = 0, over = f1;                                   // candidates in LDS; the first face left in global memory
  for (int first = f0; first < f1; first += kGraspThreads) {
    const int f = first + tid;
    Vec3 v0, v1, v2;
    const bool keep = f < f1 && load_face(verts, V, faces, f, v0, v1, v2) && in_reach(v0, v1, v2, centre, radius);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kGraspWaves; ++w) {
      before += w < wave ? s_cnt[w] : 0;
      total += s_cnt[w];
    }
    __syncthreads();                                          // (s_cnt is written again in the next round)
    if (n_lds + total > kGraspCapacity) {                     // uniform: this chunk and everything after it stay in global memory
      over = first;
      break;
    }
    if (keep) {
      const int slot = n_lds + before + __popcll(mask & ((1ull << lane) - 1ull));
      float *t = s_tri + slot * 9;
      t[0] = v0.x, t[1] = v0.y, t[2] = v0.z, t[3] = v1.x, t[4] = v1.y, t[5] = v1.z, t[6] = v2.x, t[7] = v2.y, t[8] = v2.z;
    }
    n_lds += total;
  }
  __syncthreads();

  // ---- the sweep ---------------------------------------------------------------------------------------------------------------
  float q[kGraspJoints];
  int blocked[kGraspJoints];
  bool frozen[kGraspJoints];
#pragma unroll
  for (int j = 0; j < kGraspJoints; ++j) {
    q[j] = chain[j].q0;
    blocked[j] = steps;
    frozen[j] = false;
  }
  const bool candidates = n_lds > 0 || over < f1;
  for (int step = 1; step <= steps; ++step) {
    bool moved = false;
#pragma unroll
    for (int j = 0; j < kGraspJoints; ++j) {
      if (frozen[j]) continue;
      moved = true;
      const float tried = step == steps ? chain[j].upper : chain[j].q0 + (float)step * chain[j].delta;
      if (!candidates) {                                      // nothing in reach: every try is accepted, poses are formed at the end
        q[j] = tried;
        continue;
      }
      if (tid == 0) {
        int nb = 0;
#pragma unroll
        for (int k = j; k < kGraspChain; ++k) {
          const int parent = chain[k].parent;
          const float *Rp = parent < 0 ? s_base + 3 : parent < j ? s_R[parent] : s_TR[parent];
          const float *pp = parent < 0 ? s_base : parent < j ? s_p[parent] : s_Tp[parent];
          link_pose(chain[k], Rp, pp, k == j ? tried : k < kGraspJoints ? q[k < kGraspJoints ? k : 0] : 0.f, s_TR[k], s_Tp[k]);
          if (chain[k].has_box) {
            float *box = s_box + 15 * nb++;
            for (int i = 0; i < 3; ++i)
              box[i] = s_Tp[k][i] + (s_TR[k][3 * i] * chain[k].bc[0] + s_TR[k][3 * i + 1] * chain[k].bc[1] + s_TR[k][3 * i + 2] * chain[k].bc[2]);
            for (int i = 0; i < 9; ++i) box[3 + i] = s_TR[k][i];
            for (int i = 0; i < 3; ++i) box[12 + i] = chain[k].bh[i];
          }
        }
        s_nb = nb;
      }
      __syncthreads();
      const int nb = s_nb;
      bool hit = false;
      if (nb > 0) {
        for (int i = tid; i < n_lds && !hit; i += kGraspThreads) {
          const float *t = s_tri + i * 9;
          hit = any_box_overlaps(s_box, nb, load3(t), load3(t + 3), load3(t + 6));
        }
        for (int f = over + tid; f < f1 && !hit; f += kGraspThreads) {
          Vec3 v0, v1, v2;
          if (load_face(verts, V, faces, f, v0, v1, v2) && in_reach(v0, v1, v2, centre, radius)) hit = any_box_overlaps(s_box, nb, v0, v1, v2);
        }
      }
      const unsigned long long mask = __ballot(hit);
      if (lane == 0) s_hit[wave] = mask != 0ull;
      __syncthreads();
      int any = 0;
#pragma unroll
      for (int w = 0; w < kGraspWaves; ++w) any |= s_hit[w];
      if (__builtin_amdgcn_readfirstlane(any)) {
        frozen[j] = true;
        blocked[j] = step - 1;
      } else {
        q[j] = tried;
        if (tid == 0) {
          for (int k = j; k < kGraspChain; ++k) {
            for (int i = 0; i < 9; ++i) s_R[k][i] = s_TR[k][i];
            for (int i = 0; i < 3; ++i) s_p[k][i] = s_Tp[k][i];
          }
        }
      }
    }
    if (!moved) break;
  }
  if (tid == 0) {
    if (!candidates) {
      for (int k = 0; k < kGraspChain; ++k) {
        const int parent = chain[k].parent;
        float angle = 0.f;
#pragma unroll
        for (int j = 0; j < kGraspJoints; ++j) angle = k == j ? q[j] : angle;
        link_pose(chain[k], parent < 0 ? s_base + 3 : s_R[parent], parent < 0 ? s_base : s_p[parent], angle, s_R[k], s_p[k]);
      }
    }
#pragma unroll
    for (int j = 0; j < kGraspJoints; ++j) {
      s_final[j] = (int)f32_bits(q[j]);
      s_final[kGraspJoints + j] = blocked[j];
    }
  }
  __syncthreads();

  // ---- the outputs -------------------------------------------------------------------------------------------------------------
  const long long row = g * kGraspFingers + finger;           // (grasp, finger)
  if (tid < kGraspJoints) {
    q_out[row * kGraspJoints + tid] = bits_f32((unsigned)s_final[tid]);
    blocked_out[row * kGraspJoints + tid] = s_final[kGraspJoints + tid];
  }
  if (tid < kGraspChain * 3) link_pos[row * kGraspChain * 3 + tid] = s_p[tid / 3][tid % 3];
  if (tid < kGraspChain * 9) link_rot[row * kGraspChain * 9 + tid] = s_R[tid / 9][tid % 9];
  if (tid < 3) frame_pos[row * 3 + tid] = s_p[kGraspChain - 1][tid];
  if (tid < 9) frame_rot[row * 9 + tid] = s_R[kGraspChain - 1][tid];
}

}  // namespace

int launch_grasp_close(const float *verts, int V, const int32_t *faces, const int32_t *f0, const int32_t *f1, const float *base_pos,
                       const float *base_rot, int G, const GraspHand &hand, int steps, float *q_out, int32_t *blocked_step, float *link_pos,
                       float *link_rot, float *frame_pos, float *frame_rot, hipStream_t s) {
  int launches = 0;
  for (int g0 = 0; g0 < G; g0 += kGraspPerLaunch) {
    const int n = G - g0 < kGraspPerLaunch ? G - g0 : kGraspPerLaunch;
    GraspRanges ranges = {};
    for (int i = 0; i < n; ++i) {
      ranges.f0[i] = f0[g0 + i];
      ranges.f1[i] = f1[g0 + i];
    }
    A3VT_LAUNCH(grasp_close_kernel, dim3(n * kGraspFingers), dim3(kGraspThreads), 0, s, verts, V, faces, ranges, base_pos, base_rot, g0,
                hand, steps, q_out, blocked_step, link_pos, link_rot, frame_pos, frame_rot);
    A3VT_CHECK_LAUNCH();
    ++launches;
  }
  return launches;
}

}  // namespace a3vt
