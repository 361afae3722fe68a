// scene_render.hip — looking at a result: colour, depth and primitive-index images of scenes of triangles and analytic spheres, the
// job utility/pretty_render.py gives to pyrender (512 x 512 views of the predicted mesh, of 100 000 surface samples as spheres and of
// the ground-truth mesh, per object).  The contract is a3vt_scene_render's in include/a3vt.h.
//
// THE SHADER IS NOT PYRENDER'S.  This is ray casting at pixel centres with Lambert shading under the reference's lights and camera:
// no shadows, no specular term, no vertex-normal smoothing, no blending, and nothing of the metallic-roughness model.  No image of it
// has been compared with one of pyrender's.
//
//   scene_render   one workgroup of 256 threads per 16 x 16 pixel tile of one image.  The image's faces, then its spheres, are taken
//                  256 at a time: thread t bounds primitive t (a face's bounding sphere, a sphere itself), moved to the camera frame,
//                  against the four side planes of the tile's pyramid and the depth range; the survivors are ballot-compacted into
//                  LDS (14 words a face, 5 a sphere); then every thread casts its pixel's ray at them and keeps (depth, index) of
//                  the nearest hit, the lower index among equal depths.  That rule is a total order, so neither the chunking nor the
//                  survivors' order shows.  The triangle test is touch_render.hip's, restated: edge functions d . (a x b) with the
//                  cross product formed from the vertex of the lower index to the higher in explicitly rounded steps, inclusive,
//                  two-sided, depth = (v . n) / (d . n) — with n and v formed from the vertices in index order, so that coincident
//                  copies of a face under another winding give exactly equal depths and the tie rule decides.  A sphere is hit at b - sqrt(disc), b = c . u, disc = r^2 - |c - b u|^2
//                  (u the unit ray, the eye at the origin): no difference of two large squares.  The winner is then read again by
//                  its index and shaded; a thread outside the image (a partial tile at the right or bottom edge) goes through every
//                  ballot and barrier and stores nothing.
// Barriers per chunk: one after the survivor counts (kept in two alternating rows, so a wave still adding up chunk k's cannot see chunk
// k + 1's), one after the records are written when any survived; the reads of chunk k are fenced from the writes of chunk k + 1 by
// that chunk's first barrier.  No atomics, no workspace, every float sum in a fixed order: the same bits on every call, whatever
// else is in the batch.
#include <math.h>
#include <string.h>

#include "common.h"
#include "kernels.h"

namespace a3vt {

namespace {

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

// The tile's pyramid (pixel edges; the last tiles end with the image) and the depth range, against a bounding sphere in the eye frame.
struct Frustum {
  float xl, xr, yt, yb, il, ir, it, ib, znear, zfar;
};
__device__ __forceinline__ bool frustum_keeps(const Frustum &f, V3 q, float rad) {
  const float w = -q.z;
  // generous against the rounding of the centre and the radius: the cull may keep too much, never too little
  const float rs = rad * 1.001f + 1e-6f * (fabsf(q.x) + fabsf(q.y) + fabsf(w));
  return (q.x - f.xl * w) * f.il >= -rs && (f.xr * w - q.x) * f.ir >= -rs && (q.y - f.yb * w) * f.ib >= -rs &&
         (f.yt * w - q.y) * f.it >= -rs && w + rs >= f.znear && w - rs <= f.zfar;
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

__global__ __launch_bounds__(kThreads) void scene_render_kernel(
    const float *__restrict__ verts, int V, const int32_t *__restrict__ faces, const uint8_t *__restrict__ face_rgb, int F,
    const float *__restrict__ centres, const float *__restrict__ radii, const uint8_t *__restrict__ sphere_rgb,
    const float *__restrict__ cam_pos, const float *__restrict__ cam_rot, const SceneTables tab, int img0, float tan_x, float tan_y,
    float znear, float zfar, int W, int H, int tiles_across, int tiles_per_image, uint8_t *__restrict__ rgb, float *__restrict__ depth,
    int32_t *__restrict__ prim) {
  __shared__ float rec_s[kFaceRecord][kSceneChunk];
  __shared__ int wave_n[2][kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int local = blockIdx.x / tiles_per_image, tile = blockIdx.x - local * tiles_per_image;
  const int ty = tile / tiles_across, tx = tile - ty * tiles_across;
  const long long img = (long long)img0 + local;
  const int r = ty * kTile + tid / kTile, c = tx * kTile + tid % kTile;
  const SceneRange range = tab.range[local];
  const Camera cam = load_camera(cam_pos, cam_rot, img);

  // the pixel's ray (through its centre, row 0 at the top) and its unit form for the spheres
  const float fw = (float)W, fh = (float)H;
  const V3 d = {((c + 0.5f) / fw * 2.f - 1.f) * tan_x, (1.f - (r + 0.5f) / fh * 2.f) * tan_y, -1.f};
  const float inv_len = 1.f / sqrtf(dot(d, d));
  const V3 u = {d.x * inv_len, d.y * inv_len, -inv_len};
  Frustum fr;
  fr.xl = ((float)(tx * kTile) / fw * 2.f - 1.f) * tan_x;
  fr.xr = ((float)min(tx * kTile + kTile, W) / fw * 2.f - 1.f) * tan_x;
  fr.yt = (1.f - (float)(ty * kTile) / fh * 2.f) * tan_y;
  fr.yb = (1.f - (float)min(ty * kTile + kTile, H) / fh * 2.f) * tan_y;
  fr.il = rsqrtf(1.f + fr.xl * fr.xl), fr.ir = rsqrtf(1.f + fr.xr * fr.xr);
  fr.it = rsqrtf(1.f + fr.yt * fr.yt), fr.ib = rsqrtf(1.f + fr.yb * fr.yb);
  fr.znear = znear, fr.zfar = zfar;

  float best = INFINITY;
  int best_id = -1, parity = 0;

  for (int base = range.f0; base < range.f1; base += kSceneChunk, parity ^= 1) {
    const int f = base + tid;
    bool keep = false;
    int i0 = 0, i1 = 0, i2 = 0;
    V3 a = {}, b = {}, e = {};
    if (f < range.f1) {
      i0 = faces[3ll * f], i1 = faces[3ll * f + 1], i2 = faces[3ll * f + 2];
      if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {   // (others are skipped)
        a = load3(verts, i0), b = load3(verts, i1), e = load3(verts, i2);
        if (finite3(a) && finite3(b) && finite3(e)) {
          const V3 g = {(a.x + b.x + e.x) * (1.f / 3.f), (a.y + b.y + e.y) * (1.f / 3.f), (a.z + b.z + e.z) * (1.f / 3.f)};
          const V3 da = sub(a, g), db = sub(b, g), de = sub(e, g);
          const float rad = sqrtf(fmaxf(dot(da, da), fmaxf(dot(db, db), dot(de, de))));
          keep = frustum_keeps(fr, to_eye(cam, g), rad);   // (a sum that overflowed gives a NaN or an infinity: not kept)
        }
      }
    }
    int total;
    const int slot = compact(keep, wave_n, parity, lane, wave, &total);
    if (total == 0) continue;   // (uniform)
    if (keep) {
      const V3 v0 = to_eye(cam, a), v1 = to_eye(cam, b), v2 = to_eye(cam, e);
      const V3 c0 = edge_vector(v1, v2, i1, i2), c1 = edge_vector(v2, v0, i2, i0), c2 = edge_vector(v0, v1, i0, i1);
      V3 low;
      const V3 n = plane_normal(v0, v1, v2, i0, i1, i2, &low);
      rec_s[0][slot] = c0.x, rec_s[1][slot] = c0.y, rec_s[2][slot] = c0.z;
      rec_s[3][slot] = c1.x, rec_s[4][slot] = c1.y, rec_s[5][slot] = c1.z;
      rec_s[6][slot] = c2.x, rec_s[7][slot] = c2.y, rec_s[8][slot] = c2.z;
      rec_s[9][slot] = n.x, rec_s[10][slot] = n.y, rec_s[11][slot] = n.z;
      rec_s[12][slot] = dot(low, n);
      rec_s[13][slot] = __int_as_float(f);
    }
    __syncthreads();
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
  }

  for (int base = range.s0; base < range.s1; base += kSceneChunk, parity ^= 1) {
    const int sph = base + tid;
    bool keep = false;
    V3 q = {};
    float rad = 0.f;
    if (sph < range.s1) {
      const V3 centre = load3(centres, sph);
      rad = radii[sph];
      if (finite3(centre) && isfinite(rad) && rad > 0.f) {
        q = to_eye(cam, centre);
        keep = frustum_keeps(fr, q, rad);
      }
    }
    int total;
    const int slot = compact(keep, wave_n, parity, lane, wave, &total);
    if (total == 0) continue;   // (uniform)
    if (keep) {
      rec_s[0][slot] = q.x, rec_s[1][slot] = q.y, rec_s[2][slot] = q.z;
      rec_s[3][slot] = __fmul_rn(rad, rad);
      rec_s[4][slot] = __int_as_float(F + sph);
    }
    __syncthreads();
    for (int j = 0; j < total; ++j) {
      const V3 q_j = {rec_s[0][j], rec_s[1][j], rec_s[2][j]};
      const float bq = dot(q_j, u);
      const V3 w = {__fmaf_rn(-bq, u.x, q_j.x), __fmaf_rn(-bq, u.y, q_j.y), __fmaf_rn(-bq, u.z, q_j.z)};
      const float disc = rec_s[3][j] - dot(w, w);
      if (disc >= 0.f) {
        const float t = __fmul_rn(bq - sqrtf(disc), inv_len);   // along the unit ray, then as -z of the hit (negative from inside)
        const int id = __float_as_int(rec_s[4][j]);
        if (t >= znear && t <= zfar && (t < best || (t == best && id < best_id))) best = t, best_id = id;
      }
    }
  }

  if (r >= H || c >= W) return;   // (after the last barrier)
  const long long pix = (img * H + r) * W + c;
  depth[pix] = best_id < 0 ? 0.f : best;
  if (prim) prim[pix] = best_id;
  uint8_t *out = rgb + 3 * pix;
  if (best_id < 0) {
    out[0] = tab.background[0], out[1] = tab.background[1], out[2] = tab.background[2];
    return;
  }
  // the winner again, by its index: the hit point, the unit normal towards the eye (at the origin), the base colour
  const V3 p = {d.x * best, d.y * best, -best};
  V3 n;
  const uint8_t *base_rgb;
  if (best_id < F) {
    const int i0 = faces[3ll * best_id], i1 = faces[3ll * best_id + 1], i2 = faces[3ll * best_id + 2];
    V3 low;
    n = plane_normal(to_eye(cam, load3(verts, i0)), to_eye(cam, load3(verts, i1)), to_eye(cam, load3(verts, i2)), i0, i1, i2, &low);
    const float big = fmaxf(fabsf(n.x), fmaxf(fabsf(n.y), fabsf(n.z)));   // (a small face's n . n would leave fp32's range)
    n = {n.x / big, n.y / big, n.z / big};
    const float len = sqrtf(dot(n, n)), side = dot(n, p) > 0.f ? -1.f : 1.f;
    n = {side * n.x / len, side * n.y / len, side * n.z / len};
    base_rgb = face_rgb + 3ll * best_id;
  } else {
    const int sph = best_id - F;
    const V3 q = to_eye(cam, load3(centres, sph));
    const float rad = radii[sph];
    n = {(p.x - q.x) / rad, (p.y - q.y) / rad, (p.z - q.z) / rad};
    base_rgb = sphere_rgb + 3ll * sph;
  }
  float sum = 0.f;
  for (int k = 0; k < tab.n_lights; ++k) {   // (in table order)
    const V3 l = sub(to_eye(cam, {tab.light[k][0], tab.light[k][1], tab.light[k][2]}), p);
    const float len2 = dot(l, l), len = sqrtf(len2);
    sum += tab.light[k][3] * fmaxf(0.f, dot(n, l) / len) / len2;
  }
  const float shade = tab.ambient + sum * 0.318309886183790672f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = (uint8_t)floorf(fminf(fmaxf((float)base_rgb[ch] * shade, 0.f), 255.f) + 0.5f);
}

}  // namespace

int launch_scene_render(const float *verts, int V, const int32_t *faces, const uint8_t *face_rgb, int F, const float *centres,
                        const float *radii, const uint8_t *sphere_rgb, const SceneRange *ranges, const float *cam_pos,
                        const float *cam_rot, int I, float yfov, float znear, float zfar, int W, int H, const float *lights, int L,
                        float ambient, const uint8_t *background, uint8_t *rgb, float *depth, int32_t *prim, hipStream_t s) {
  const double tan_half = tan(0.5 * (double)yfov);
  const float tan_y = (float)tan_half, tan_x = (float)(tan_half * (double)W / (double)H);
  const int tiles_across = cdiv(W, kTile), tiles_per_image = tiles_across * cdiv(H, kTile);
  SceneTables tab;
  memset(&tab, 0, sizeof(tab));
  for (int k = 0; k < L; ++k) memcpy(tab.light[k], lights + 4 * k, 4 * sizeof(float));
  tab.n_lights = L, tab.ambient = ambient;
  memcpy(tab.background, background, 3);
  int launches = 0;
  for (int img0 = 0; img0 < I; img0 += kSceneImagesPerLaunch, ++launches) {
    const int n = I - img0 < kSceneImagesPerLaunch ? I - img0 : kSceneImagesPerLaunch;
    memcpy(tab.range, ranges + img0, n * sizeof(SceneRange));
    A3VT_LAUNCH(scene_render_kernel, dim3((unsigned)n * (unsigned)tiles_per_image), dim3(kThreads), 0, s, verts, V, faces, face_rgb, F,
                centres, radii, sphere_rgb, cam_pos, cam_rot, tab, img0, tan_x, tan_y, znear, zfar, W, H, tiles_across, tiles_per_image,
                rgb, depth, prim);
    A3VT_CHECK_LAUNCH();
  }
  return launches;
}

}  // namespace a3vt
