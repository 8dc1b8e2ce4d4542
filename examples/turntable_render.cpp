// turntable_render.cpp — one mesh of a scene turned about the vertical axis through its centre, posed on the device from
// one 3x4 matrix per mesh (ptamd_scene_rig, include/ptamd.h), one image per step.
//   g++ -std=c++17 -Iinclude examples/turntable_render.cpp -Lcuda-pathtracer_amd -lptamd
//       -Wl,-rpath,$PWD/cuda-pathtracer_amd -o turntable_render
//   ./turntable_render assets/crate_land.scene 960 540 16 8 0 turn     (16 frames per step, 8 steps, mesh 0: turn_0.png ...)
#include "ptamd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define CHECK(call)                                                                     \
  do {                                                                                  \
    int rc_ = (call);                                                                   \
    if (rc_ != PTAMD_OK) { std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ptamd_get_last_error()); return 1; } \
  } while (0)

int main(int argc, char** argv)
{
  if (argc < 8) { std::fprintf(stderr, "usage: %s SCENE WIDTH HEIGHT FRAMES STEPS MESH OUT_PREFIX\n", argv[0]); return 2; }
  const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]), frames = (uint32_t)std::atoi(argv[4]);
  const int steps = std::atoi(argv[5]);
  const uint32_t mesh = (uint32_t)std::atoi(argv[6]);
  ptamd_host_scene* hs = nullptr;
  CHECK(ptamd_host_scene_load(argv[1], 0, &hs));
  ptamd_scene_desc desc;
  ptamd_camera cam;
  CHECK(ptamd_host_scene_desc(hs, &desc));
  CHECK(ptamd_host_scene_camera(hs, &cam));
  if (mesh >= desc.n_meshes || desc.mesh_sizes[mesh] == 0) { std::fprintf(stderr, "the scene has %u meshes\n", desc.n_meshes); return 2; }
  ptamd_context* ctx = nullptr;
  CHECK(ptamd_create(0, &ctx));
  uint32_t scene_id = 0, cubemap_id = 0;
  float cube[24];
  CHECK(ptamd_cubemap_from_color(0x131b23, cube));
  CHECK(ptamd_upload_scene(ctx, &desc, &scene_id));
  CHECK(ptamd_upload_cubemap(ctx, cube, 1, &cubemap_id));
  ptamd_scene_rig* rig = nullptr;   // the rest pose is the scene as loaded, the groups are its meshes
  CHECK(ptamd_scene_rig_create(ctx, scene_id, desc.faces, desc.n_faces, desc.mesh_sizes, desc.n_meshes, &rig));
  // the pivot: the centre of the mesh's vertices
  uint32_t first = 0;
  for (uint32_t m = 0; m < mesh; ++m) first += desc.mesh_sizes[m];
  double c[3] = { 0, 0, 0 };
  for (uint32_t i = first; i < first + desc.mesh_sizes[mesh]; ++i)
    for (int k = 0; k < 3; ++k) { c[0] += desc.faces[i].vertices[k].x; c[1] += desc.faces[i].vertices[k].y; c[2] += desc.faces[i].vertices[k].z; }
  for (double& v : c) v /= 3.0 * desc.mesh_sizes[mesh];
  void *surface = nullptr, *tfb = nullptr;
  CHECK(ptamd_device_alloc(ctx, (size_t)w * h * 4, &surface));
  CHECK(ptamd_device_alloc(ctx, (size_t)w * h * 12, &tfb));
  std::vector<float> t((size_t)desc.n_meshes * 12, 0.0f);
  std::vector<unsigned char> px((size_t)w * h * 4), rgb((size_t)w * h * 3);
  for (int s = 0; s < steps; ++s) {
    for (uint32_t m = 0; m < desc.n_meshes; ++m) { t[m * 12 + 0] = 1.0f; t[m * 12 + 5] = 1.0f; t[m * 12 + 10] = 1.0f; }   // identity
    const double a = 6.283185307179586 * s / steps, ca = std::cos(a), sa = std::sin(a);
    float* r = &t[(size_t)mesh * 12];   // x' = R (x - c) + c, a rotation about y: its own normal matrix
    r[0] = (float)ca; r[2] = (float)sa; r[8] = (float)-sa; r[10] = (float)ca;
    r[3] = (float)(c[0] - (ca * c[0] + sa * c[2])); r[7] = 0.0f; r[11] = (float)(c[2] - (-sa * c[0] + ca * c[2]));
    ptamd_scene_rig_pose_desc pose = { rig, t.data(), nullptr, desc.n_meshes, nullptr };
    CHECK(ptamd_scene_rig_pose(ctx, &pose));   // asynchronous; the launch below is ordered behind it
    ptamd_launch l = {};
    l.surface_rgba8 = surface; l.temporal_framebuffer = static_cast<float*>(tfb); l.camera = cam;
    l.scene_id = scene_id; l.cubemap_id = cubemap_id; l.width = w; l.height = h; l.row_end = h;
    l.frame_nb = 1; l.frame_count = frames; l.bounces = 3; l.reset_accumulation = 1;
    CHECK(ptamd_raytrace_ex(ctx, &l));
    CHECK(ptamd_device_to_host(ctx, px.data(), surface, px.size(), nullptr));
    for (size_t i = 0; i < (size_t)w * h; ++i) { rgb[i * 3] = px[i * 4]; rgb[i * 3 + 1] = px[i * 4 + 1]; rgb[i * 3 + 2] = px[i * 4 + 2]; }
    const std::string out = std::string(argv[7]) + "_" + std::to_string(s) + ".png";
    CHECK(ptamd_image_save_png(out.c_str(), rgb.data(), (int32_t)w, (int32_t)h, 3));
  }
  CHECK(ptamd_scene_rig_destroy(ctx, rig));   // before its context
  ptamd_device_free(ctx, surface);
  ptamd_device_free(ctx, tfb);
  ptamd_destroy(ctx);
  ptamd_host_scene_free(hs);
  return 0;
}
