// posed_render.hip — the posed hand in the vision scene (simulator/rendering/vision_renderer.py::update_hand + render): colour, depth
// and primitive images of scenes of INSTANCES.  An instance is a part — a face range of a shared template table —, a rigid pose and a
// colour; the object of an image is an instance under the identity, the Allegro hand 21 more.  The contract is
// a3vt_scene_render_posed's in include/a3vt.h.  THE SHADER IS NOT PYRENDER'S: it is scene_render.hip's, word for word (scene_dev.h).
//
//   scene_render_posed   one workgroup of 256 threads per 16 x 16 pixel tile of one image.
//                        Phase 1: the image's instances, 256 at a time.  Thread t checks instance t (part id in range, pose finite)
//                        and bounds it — the part's sphere, its centre posed like a vertex and its radius scaled by the Frobenius
//                        norm of R, which bounds |R v| / |v| for ANY matrix — against the tile's pyramid and the depth range;
//                        survivors are ballot-compacted into LDS in instance order.
//                        Phase 2: a uniform loop over the survivors.  Each walks its part's faces 256 at a time: thread t poses its
//                        face's three vertices (pose_vertex: three fused multiply-adds per row), and from there runs scene_render's
//                        own cull, record, cast and tie code.  An instance keeps its nearest hit (the lower face index among equal
//                        depths); it replaces the pixel's only when STRICTLY nearer, so among equal depths the lower instance wins.
//   pose_parts           the materialised formulation: a workgroup per instance writes the posed vertices (pose_vertex again), the
//                        faces re-based onto them and a colour per face.  scene_render on that output gives posed_render's bits.
// A composed template -> eye transform would save the world step; it is not used, because the rule above is what makes the result
// checkable bit for bit against scene_render.  No atomics, no workspace, no host synchronisation; an image depends on nothing else in
// the batch.  Barriers: scene_dev.h's compact() protocol (two alternating count rows), one more after the survivors' list is written.
#include <math.h>
#include <string.h>

#include "common.h"
#include "kernels.h"
#include "scene_dev.h"

namespace a3vt {

namespace {

using namespace scene_dev;

__global__ __launch_bounds__(kThreads) void scene_render_posed_kernel(
    const float *__restrict__ part_verts, int PV, const int32_t *__restrict__ part_faces, const int32_t *__restrict__ inst_part,
    const float *__restrict__ inst_pos, const float *__restrict__ inst_rot, const uint8_t *__restrict__ inst_rgb,
    const float *__restrict__ cam_pos, const float *__restrict__ cam_rot, const PosedTables tab, int img0, float tan_x, float tan_y,
    float znear, float zfar, int W, int H, int tiles_across, int tiles_per_image, uint8_t *__restrict__ rgb, float *__restrict__ depth,
    int32_t *__restrict__ prim_inst, int32_t *__restrict__ prim_face) {
  __shared__ float rec_s[kFaceRecord][kSceneChunk];
  __shared__ int wave_n[2][kWaves];
  __shared__ int inst_s[kSceneChunk];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int local = blockIdx.x / tiles_per_image, tile = blockIdx.x - local * tiles_per_image;
  const int ty = tile / tiles_across, tx = tile - ty * tiles_across;
  const long long img = (long long)img0 + local;
  const int r = ty * kTile + tid / kTile, c = tx * kTile + tid % kTile;
  const int n0 = tab.inst0[local], n1 = tab.inst1[local];
  const Camera cam = load_camera(cam_pos, cam_rot, img);

  const float fw = (float)W, fh = (float)H;
  const V3 d = pixel_ray(r, c, fw, fh, tan_x, tan_y);
  const Frustum fr = tile_frustum(tx, ty, W, H, fw, fh, tan_x, tan_y, znear, zfar);

  float best = INFINITY;
  int best_inst = -1, best_face = -1, parity = 0;

  for (int ibase = n0; ibase < n1; ibase += kSceneChunk) {
    // Phase 1: thread t bounds instance ibase + t
    const int n = ibase + tid;
    bool keep = false;
    if (n < n1) {
      const int part = inst_part[n];
      if ((unsigned)part < (unsigned)tab.n_parts) {   // (others are skipped, as a whole)
        const Pose q = load_pose(inst_pos, inst_rot, n);
        if (finite_pose(q)) {
          float norm2 = 0.f;
#pragma unroll
          for (int k = 0; k < 9; ++k) norm2 = fmaf(q.r[k], q.r[k], norm2);
          const V3 w = pose_vertex(q, {tab.bound[part][0], tab.bound[part][1], tab.bound[part][2]});
          // |R v| <= |R|_F |v|; generous against the rounding of the norm and of the posed centre
          const float rad = tab.bound[part][3] * sqrtf(norm2) * 1.0001f + 1e-6f * (fabsf(w.x) + fabsf(w.y) + fabsf(w.z));
          const V3 e = to_eye(cam, w);
          // a bound that left fp32's range bounds nothing: the faces are then tested one by one
          keep = !(finite3(e) && isfinite(rad)) || frustum_keeps(fr, e, rad);
        }
      }
    }
    int survivors;
    const int at = compact(keep, wave_n, parity, lane, wave, &survivors);
    parity ^= 1;
    if (survivors == 0) continue;   // (uniform)
    if (keep) inst_s[at] = n;
    __syncthreads();

    // Phase 2: the survivors in instance order, every thread in step
    for (int j = 0; j < survivors; ++j) {
      const int inst = inst_s[j];
      const int part = inst_part[inst];
      const Pose q = load_pose(inst_pos, inst_rot, inst);
      const int f0 = tab.face0[part], f1 = tab.face1[part];
      float near = INFINITY;
      int near_face = -1;
      for (int base = f0; base < f1; base += kSceneChunk, parity ^= 1) {
        const int f = base + tid;
        bool keep_face = false;
        int i0 = 0, i1 = 0, i2 = 0;
        V3 a = {}, b = {}, e = {};
        if (f < f1) {
          i0 = part_faces[3ll * f], i1 = part_faces[3ll * f + 1], i2 = part_faces[3ll * f + 2];
          if ((unsigned)i0 < (unsigned)PV && (unsigned)i1 < (unsigned)PV && (unsigned)i2 < (unsigned)PV) {   // (others are skipped)
            a = pose_vertex(q, load3(part_verts, i0)), b = pose_vertex(q, load3(part_verts, i1)), e = pose_vertex(q, load3(part_verts, i2));
            if (finite3(a) && finite3(b) && finite3(e)) keep_face = face_kept(fr, cam, a, b, e);
          }
        }
        int total;
        const int slot = compact(keep_face, wave_n, parity, lane, wave, &total);
        if (total == 0) continue;   // (uniform)
        if (keep_face) face_record(rec_s, slot, cam, a, b, e, i0, i1, i2, f);
        __syncthreads();
        cast_faces(rec_s, total, d, znear, zfar, &near, &near_face);
      }
      if (near_face >= 0 && near < best) best = near, best_inst = inst, best_face = near_face;   // (a tie stays with the lower instance)
    }
  }

  if (r >= H || c >= W) return;   // (after the last barrier)
  const long long pix = (img * H + r) * W + c;
  depth[pix] = best_inst < 0 ? 0.f : best;
  if (prim_inst) prim_inst[pix] = best_inst, prim_face[pix] = best_face;
  uint8_t *out = rgb + 3 * pix;
  if (best_inst < 0) {
    out[0] = tab.background[0], out[1] = tab.background[1], out[2] = tab.background[2];
    return;
  }
  // the winner again, by its indices: the hit point, the unit normal towards the eye (at the origin), the instance's colour
  const V3 p = {d.x * best, d.y * best, -best};
  const Pose q = load_pose(inst_pos, inst_rot, best_inst);
  const int i0 = part_faces[3ll * best_face], i1 = part_faces[3ll * best_face + 1], i2 = part_faces[3ll * best_face + 2];
  const V3 n = face_normal(cam, pose_vertex(q, load3(part_verts, i0)), pose_vertex(q, load3(part_verts, i1)),
                           pose_vertex(q, load3(part_verts, i2)), i0, i1, i2, p);
  shade(tab, cam, p, n, inst_rgb + 3ll * best_inst, out);
}

// A workgroup per instance: its part's vertices posed, its part's faces re-based onto them, the instance's colour per face.  The
// output ranges come from vert_base / face_base; an instance whose range does not match its part's (or whose part id is out of range)
// writes nothing, and no index leaves [0, TV) or [0, TF).
__global__ __launch_bounds__(kThreads) void pose_parts_kernel(const float *__restrict__ part_verts, const int32_t *__restrict__ part_faces,
                                                              const PosedParts tab, const int32_t *__restrict__ inst_part,
                                                              const float *__restrict__ inst_pos, const float *__restrict__ inst_rot,
                                                              const uint8_t *__restrict__ inst_rgb, const int32_t *__restrict__ vert_base,
                                                              const int32_t *__restrict__ face_base, float *__restrict__ verts_out, int TV,
                                                              int32_t *__restrict__ faces_out, uint8_t *__restrict__ face_rgb_out, int TF) {
  const int inst = blockIdx.x, tid = threadIdx.x;
  const int part = inst_part[inst];
  if ((unsigned)part >= (unsigned)tab.n_parts) return;
  const int v0 = tab.vert0[part], nv = tab.vert1[part] - v0, f0 = tab.face0[part], nf = tab.face1[part] - f0;
  const int ov = vert_base[inst], of = face_base[inst];
  if (ov < 0 || of < 0 || vert_base[inst + 1] - ov != nv || face_base[inst + 1] - of != nf || ov > TV - nv || of > TF - nf) return;
  const Pose q = load_pose(inst_pos, inst_rot, inst);
  for (int i = tid; i < nv; i += kThreads) {
    const V3 w = pose_vertex(q, load3(part_verts, v0 + i));
    verts_out[3ll * (ov + i)] = w.x, verts_out[3ll * (ov + i) + 1] = w.y, verts_out[3ll * (ov + i) + 2] = w.z;
  }
  const uint8_t red = inst_rgb[3ll * inst], green = inst_rgb[3ll * inst + 1], blue = inst_rgb[3ll * inst + 2];
  for (int i = tid; i < nf; i += kThreads) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int index = part_faces[3ll * (f0 + i) + k] - v0;
      faces_out[3ll * (of + i) + k] = (unsigned)index < (unsigned)nv ? ov + index : -1;   // (-1: scene_render skips such a face)
    }
    face_rgb_out[3ll * (of + i)] = red, face_rgb_out[3ll * (of + i) + 1] = green, face_rgb_out[3ll * (of + i) + 2] = blue;
  }
}

}  // namespace

int launch_scene_render_posed(const float *part_verts, int PV, const int32_t *part_faces, const int32_t *part_face_offset,
                              const float *part_bound, int P, const int32_t *inst_part, const float *inst_pos, const float *inst_rot,
                              const uint8_t *inst_rgb, const int32_t *inst_offset, const float *cam_pos, const float *cam_rot, int I,
                              float yfov, float znear, float zfar, int W, int H, const float *lights, int L, float ambient,
                              const uint8_t *background, uint8_t *rgb, float *depth, int32_t *prim_inst, int32_t *prim_face,
                              hipStream_t s) {
  const double tan_half = tan(0.5 * (double)yfov);
  const float tan_y = (float)tan_half, tan_x = (float)(tan_half * (double)W / (double)H);
  const int tiles_across = cdiv(W, kTile), tiles_per_image = tiles_across * cdiv(H, kTile);
  PosedTables tab;
  memset(&tab, 0, sizeof(tab));
  for (int p = 0; p < P; ++p) {
    tab.face0[p] = part_face_offset[p], tab.face1[p] = part_face_offset[p + 1];
    memcpy(tab.bound[p], part_bound + 4 * p, 4 * sizeof(float));
  }
  for (int k = 0; k < L; ++k) memcpy(tab.light[k], lights + 4 * k, 4 * sizeof(float));
  tab.n_parts = P, tab.n_lights = L, tab.ambient = ambient;
  memcpy(tab.background, background, 3);
  int launches = 0;
  for (int img0 = 0; img0 < I; img0 += kSceneImagesPerLaunch, ++launches) {
    const int n = I - img0 < kSceneImagesPerLaunch ? I - img0 : kSceneImagesPerLaunch;
    for (int i = 0; i < n; ++i) tab.inst0[i] = inst_offset[img0 + i], tab.inst1[i] = inst_offset[img0 + i + 1];
    A3VT_LAUNCH(scene_render_posed_kernel, dim3((unsigned)n * (unsigned)tiles_per_image), dim3(kThreads), 0, s, part_verts, PV,
                part_faces, inst_part, inst_pos, inst_rot, inst_rgb, cam_pos, cam_rot, tab, img0, tan_x, tan_y, znear, zfar, W, H,
                tiles_across, tiles_per_image, rgb, depth, prim_inst, prim_face);
    A3VT_CHECK_LAUNCH();
  }
  return launches;
}

int launch_pose_parts(const float *part_verts, const int32_t *part_faces, const int32_t *part_vert_offset, const int32_t *part_face_offset,
                      int P, const int32_t *inst_part, const float *inst_pos, const float *inst_rot, const uint8_t *inst_rgb, int N,
                      const int32_t *vert_base, const int32_t *face_base, float *verts_out, int TV, int32_t *faces_out,
                      uint8_t *face_rgb_out, int TF, hipStream_t s) {
  if (N == 0) return 0;
  PosedParts tab;
  memset(&tab, 0, sizeof(tab));
  for (int p = 0; p < P; ++p) {
    tab.vert0[p] = part_vert_offset[p], tab.vert1[p] = part_vert_offset[p + 1];
    tab.face0[p] = part_face_offset[p], tab.face1[p] = part_face_offset[p + 1];
  }
  tab.n_parts = P;
  A3VT_LAUNCH(pose_parts_kernel, dim3((unsigned)N), dim3(kThreads), 0, s, part_verts, part_faces, tab, inst_part, inst_pos, inst_rot,
              inst_rgb, vert_base, face_base, verts_out, TV, faces_out, face_rgb_out, TF);
  A3VT_CHECK_LAUNCH();
  return 1;
}

}  // namespace a3vt
