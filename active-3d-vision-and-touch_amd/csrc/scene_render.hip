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
#include "scene_dev.h"   // the vectors, camera, cull, compaction, face record, cast and shading: shared with posed_render.hip

namespace a3vt {

namespace {

using namespace scene_dev;

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
  const V3 d = pixel_ray(r, c, fw, fh, tan_x, tan_y);
  const float inv_len = 1.f / sqrtf(dot(d, d));
  const V3 u = {d.x * inv_len, d.y * inv_len, -inv_len};
  const Frustum fr = tile_frustum(tx, ty, W, H, fw, fh, tan_x, tan_y, znear, zfar);

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
        if (finite3(a) && finite3(b) && finite3(e)) keep = face_kept(fr, cam, a, b, e);
      }
    }
    int total;
    const int slot = compact(keep, wave_n, parity, lane, wave, &total);
    if (total == 0) continue;   // (uniform)
    if (keep) face_record(rec_s, slot, cam, a, b, e, i0, i1, i2, f);
    __syncthreads();
    cast_faces(rec_s, total, d, znear, zfar, &best, &best_id);
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
    n = face_normal(cam, load3(verts, i0), load3(verts, i1), load3(verts, i2), i0, i1, i2, p);
    base_rgb = face_rgb + 3ll * best_id;
  } else {
    const int sph = best_id - F;
    const V3 q = to_eye(cam, load3(centres, sph));
    const float rad = radii[sph];
    n = {(p.x - q.x) / rad, (p.y - q.y) / rad, (p.z - q.z) / rad};
    base_rgb = sphere_rgb + 3ll * sph;
  }
  shade(tab, cam, p, n, base_rgb, out);
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
