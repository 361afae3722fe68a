// scene_dev.h — the device code of the ray caster that scene_render.hip (triangles and spheres from shared tables) and
// posed_render.hip (rigid instances of template parts) both run: the vectors with their explicitly rounded products, the camera, the
// pixel's ray, the tile's pyramid and its cull, the ballot compaction, a face's record, the cast over a chunk's records with the tie
// rule, and the shading.  One definition each, so that the two kernels cannot drift: posed_render's images equal scene_render's on
// the materialised triangles bit for bit (tests/test_gpu_posed_render.py), and that holds only while both run these functions.
#pragma once
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace a3vt {
namespace scene_dev {

constexpr int kTile = 16, kThreads = kTile * kTile;
static_assert(kThreads == kSceneChunk, "a thread bounds one primitive of a chunk");
constexpr int kFaceRecord = 14;   // c0, c1, c2 (the edge functions' vectors), n, v0 . n, the face's index
constexpr int kWaves = kThreads / kWave;

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// Explicitly rounded (no contraction the compiler may choose differently from one call site to the next): what makes the edge
// functions of a shared edge equal in magnitude in both faces.
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {__fmaf_rn(a.y, b.z, -__fmul_rn(a.z, b.y)), __fmaf_rn(a.z, b.x, -__fmul_rn(a.x, b.z)),
          __fmaf_rn(a.x, b.y, -__fmul_rn(a.y, b.x))};
}
__device__ __forceinline__ float dot(V3 a, V3 b) { return __fmaf_rn(a.x, b.x, __fmaf_rn(a.y, b.y, __fmul_rn(a.z, b.z))); }
__device__ __forceinline__ V3 edge_vector(V3 a, V3 b, int ia, int ib) {   // a x b, formed lower index first
  if (ia <= ib) return cross(a, b);
  const V3 c = cross(b, a);
  return {-c.x, -c.y, -c.z};
}
// The plane's normal (v1 - v0) x (v2 - v0) with the vertices taken in the order of their indices, and the vertex of the lowest index:
// copies of one triangle under another winding or rotation (add_faces' (a, c, b) and (c, b, a)) get the same bits, hence exactly the
// same depth at every pixel, and the tie rule decides between them.  Two-sided casting does not care for the sign.
__device__ __forceinline__ V3 plane_normal(V3 v0, V3 v1, V3 v2, int i0, int i1, int i2, V3 *lowest) {
  if (i1 < i0) {
    const V3 t = v0;
    v0 = v1, v1 = t;
    const int k = i0;
    i0 = i1, i1 = k;
  }
  if (i2 < i1) {
    const V3 t = v1;
    v1 = v2, v2 = t;
    i1 = i2;   // (i2 is not read again)
    if (i1 < i0) {
      const V3 s = v0;
      v0 = v1, v1 = s;
    }
  }
  *lowest = v0;
  return cross(sub(v1, v0), sub(v2, v0));
}
__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ __forceinline__ V3 load3(const float *p, long long i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

// A template vertex under a rigid pose (R row-major, p): per row ONE chain of three fused multiply-adds that ends in p.  This is the
// whole of posed_render's rule before `to_eye`; a3vt_pose_parts writes exactly these values out.
struct Pose {
  float r[9], p[3];
};
__device__ __forceinline__ Pose load_pose(const float *pos, const float *rot, long long i) {
  Pose q;
#pragma unroll
  for (int k = 0; k < 9; ++k) q.r[k] = rot[9 * i + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) q.p[k] = pos[3 * i + k];
  return q;
}
__device__ __forceinline__ bool finite_pose(const Pose &q) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) ok = ok && isfinite(q.r[k]);
  return ok && isfinite(q.p[0]) && isfinite(q.p[1]) && isfinite(q.p[2]);
}
__device__ __forceinline__ V3 pose_vertex(const Pose &q, V3 v) {
  return {__fmaf_rn(q.r[0], v.x, __fmaf_rn(q.r[1], v.y, __fmaf_rn(q.r[2], v.z, q.p[0]))),
          __fmaf_rn(q.r[3], v.x, __fmaf_rn(q.r[4], v.y, __fmaf_rn(q.r[5], v.z, q.p[1]))),
          __fmaf_rn(q.r[6], v.x, __fmaf_rn(q.r[7], v.y, __fmaf_rn(q.r[8], v.z, q.p[2])))};
}

// The camera's pose matrix as pretty_render.py builds it: rotation C (row-major) and position p; it looks down its own -z.
struct Camera {
  float c[9], p[3];
};
__device__ __forceinline__ Camera load_camera(const float *cam_pos, const float *cam_rot, long long img) {
  Camera cam;
#pragma unroll
  for (int i = 0; i < 9; ++i) cam.c[i] = cam_rot[9 * img + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) cam.p[i] = cam_pos[3 * img + i];
  return cam;
}
__device__ __forceinline__ V3 to_eye(const Camera &cam, V3 w) {   // C^T (w - p)
  const V3 d = {w.x - cam.p[0], w.y - cam.p[1], w.z - cam.p[2]};
  return {dot({cam.c[0], cam.c[3], cam.c[6]}, d), dot({cam.c[1], cam.c[4], cam.c[7]}, d), dot({cam.c[2], cam.c[5], cam.c[8]}, d)};
}

// The pixel's ray through its centre, row 0 at the top.
__device__ __forceinline__ V3 pixel_ray(int r, int c, float fw, float fh, float tan_x, float tan_y) {
  return {((c + 0.5f) / fw * 2.f - 1.f) * tan_x, (1.f - (r + 0.5f) / fh * 2.f) * tan_y, -1.f};
}

// The tile's pyramid (pixel edges; the last tiles end with the image) and the depth range, against a bounding sphere in the eye frame.
struct Frustum {
  float xl, xr, yt, yb, il, ir, it, ib, znear, zfar;
};
__device__ __forceinline__ Frustum tile_frustum(int tx, int ty, int W, int H, float fw, float fh, float tan_x, float tan_y, float znear,
                                                float zfar) {
  Frustum fr;
  fr.xl = ((float)(tx * kTile) / fw * 2.f - 1.f) * tan_x;
  fr.xr = ((float)min(tx * kTile + kTile, W) / fw * 2.f - 1.f) * tan_x;
  fr.yt = (1.f - (float)(ty * kTile) / fh * 2.f) * tan_y;
  fr.yb = (1.f - (float)min(ty * kTile + kTile, H) / fh * 2.f) * tan_y;
  fr.il = rsqrtf(1.f + fr.xl * fr.xl), fr.ir = rsqrtf(1.f + fr.xr * fr.xr);
  fr.it = rsqrtf(1.f + fr.yt * fr.yt), fr.ib = rsqrtf(1.f + fr.yb * fr.yb);
  fr.znear = znear, fr.zfar = zfar;
  return fr;
}
__device__ __forceinline__ bool frustum_keeps(const Frustum &f, V3 q, float rad) {
  const float w = -q.z;
  // generous against the rounding of the centre and the radius: the cull may keep too much, never too little
  const float rs = rad * 1.001f + 1e-6f * (fabsf(q.x) + fabsf(q.y) + fabsf(w));
  return (q.x - f.xl * w) * f.il >= -rs && (f.xr * w - q.x) * f.ir >= -rs && (q.y - f.yb * w) * f.ib >= -rs &&
         (f.yt * w - q.y) * f.it >= -rs && w + rs >= f.znear && w - rs <= f.zfar;
}
// A face of finite world vertices: its bounding sphere about the centroid against the tile.
__device__ __forceinline__ bool face_kept(const Frustum &fr, const Camera &cam, V3 a, V3 b, V3 e) {
  const V3 g = {(a.x + b.x + e.x) * (1.f / 3.f), (a.y + b.y + e.y) * (1.f / 3.f), (a.z + b.z + e.z) * (1.f / 3.f)};
  const V3 da = sub(a, g), db = sub(b, g), de = sub(e, g);
  const float rad = sqrtf(fmaxf(dot(da, da), fmaxf(dot(db, db), dot(de, de))));
  return frustum_keeps(fr, to_eye(cam, g), rad);   // (a sum that overflowed gives a NaN or an infinity: not kept)
}

// Survivors' slots: this thread's slot when it keeps its primitive (order preserved), and the chunk's total.  All 256 threads call it.
__device__ __forceinline__ int compact(bool keep, int (*wave_n)[kWaves], int parity, int lane, int wave, int *total) {
  const unsigned long long vote = __ballot(keep);
  if (lane == 0) wave_n[parity][wave] = __popcll(vote);
  __syncthreads();
  int slot = __popcll(vote & ((1ull << lane) - 1ull)), sum = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) slot += wave_n[parity][w];
    sum += wave_n[parity][w];
  }
  *total = sum;
  return slot;
}

// A kept face's record: world vertices a, b, e of the indices i0, i1, i2, and the index `id` the tie rule orders by.
__device__ __forceinline__ void face_record(float (*rec_s)[kSceneChunk], int slot, const Camera &cam, V3 a, V3 b, V3 e, int i0, int i1,
                                            int i2, int id) {
  const V3 v0 = to_eye(cam, a), v1 = to_eye(cam, b), v2 = to_eye(cam, e);
  const V3 c0 = edge_vector(v1, v2, i1, i2), c1 = edge_vector(v2, v0, i2, i0), c2 = edge_vector(v0, v1, i0, i1);
  V3 low;
  const V3 n = plane_normal(v0, v1, v2, i0, i1, i2, &low);
  rec_s[0][slot] = c0.x, rec_s[1][slot] = c0.y, rec_s[2][slot] = c0.z;
  rec_s[3][slot] = c1.x, rec_s[4][slot] = c1.y, rec_s[5][slot] = c1.z;
  rec_s[6][slot] = c2.x, rec_s[7][slot] = c2.y, rec_s[8][slot] = c2.z;
  rec_s[9][slot] = n.x, rec_s[10][slot] = n.y, rec_s[11][slot] = n.z;
  rec_s[12][slot] = dot(low, n);
  rec_s[13][slot] = __int_as_float(id);
}
// The ray d against the chunk's `total` records: the nearest hit in the depth range, the lower index among equal depths.
__device__ __forceinline__ void cast_faces(const float (*rec_s)[kSceneChunk], int total, V3 d, float znear, float zfar, float *best_t,
                                           int *best_index) {
  float best = *best_t;
  int best_id = *best_index;
  for (int j = 0; j < total; ++j) {   // (every lane reads the same LDS word: a broadcast)
    const float u0 = dot(d, {rec_s[0][j], rec_s[1][j], rec_s[2][j]});
    const float u1 = dot(d, {rec_s[3][j], rec_s[4][j], rec_s[5][j]});
    const float u2 = dot(d, {rec_s[6][j], rec_s[7][j], rec_s[8][j]});
    if ((u0 >= 0.f && u1 >= 0.f && u2 >= 0.f) || (u0 <= 0.f && u1 <= 0.f && u2 <= 0.f)) {
      const float t = __fdiv_rn(rec_s[12][j], dot(d, {rec_s[9][j], rec_s[10][j], rec_s[11][j]}));
      const int id = __float_as_int(rec_s[13][j]);
      // (a NaN, from a face seen edge-on, fails the range)
      if (t >= znear && t <= zfar && (t < best || (t == best && id < best_id))) best = t, best_id = id;
    }
  }
  *best_t = best, *best_index = best_id;
}

// The winning face's unit normal turned towards the eye (at the origin), from its world vertices read again; p is the hit point.
__device__ __forceinline__ V3 face_normal(const Camera &cam, V3 a, V3 b, V3 e, int i0, int i1, int i2, V3 p) {
  V3 low;
  V3 n = plane_normal(to_eye(cam, a), to_eye(cam, b), to_eye(cam, e), i0, i1, i2, &low);
  const float big = fmaxf(fabsf(n.x), fmaxf(fabsf(n.y), fabsf(n.z)));   // (a small face's n . n would leave fp32's range)
  n = {n.x / big, n.y / big, n.z / big};
  const float len = sqrtf(dot(n, n)), side = dot(n, p) > 0.f ? -1.f : 1.f;
  return {side * n.x / len, side * n.y / len, side * n.z / len};
}
// Lambert shading of the hit point p with the unit normal n and the base colour: Tables holds light, n_lights and ambient.
template <class Tables>
__device__ __forceinline__ void shade(const Tables &tab, const Camera &cam, V3 p, V3 n, const uint8_t *base_rgb, uint8_t *out) {
  float sum = 0.f;
  for (int k = 0; k < tab.n_lights; ++k) {   // (in table order)
    const V3 l = sub(to_eye(cam, {tab.light[k][0], tab.light[k][1], tab.light[k][2]}), p);
    const float len2 = dot(l, l), len = sqrtf(len2);
    sum += tab.light[k][3] * fmaxf(0.f, dot(n, l) / len) / len2;
  }
  const float level = tab.ambient + sum * 0.318309886183790672f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = (uint8_t)floorf(fminf(fmaxf((float)base_rgb[ch] * level, 0.f), 255.f) + 0.5f);
}

}  // namespace scene_dev
}  // namespace a3vt
