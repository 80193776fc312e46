/* A host in plain C99 over include/halart.h: the call sequence the reference's application runs against HalaRenderer
 * (src/rt_renderer.rs: new -> [set_envmap] -> set_scene -> commit -> { update -> render }* -> save_images), with the scene read by the
 * library's own glTF loader (what cpu::HalaScene::new(path) is in the reference).  No Python, no torch, no C++ on this side.
 *
 *   cc -std=c99 -Iinclude examples/render_gltf.c -Lhala-renderer_amd/lib -lhalart -Wl,-rpath,$PWD/hala-renderer_amd/lib -o render_gltf
 *   ./render_gltf scene.gltf out/frame 640 360 16 [env.hdr|env.exr|env.pfm [rotation_degrees [two-level]]] [--clip N --time T [--shutter T2]]
 *
 * A last argument "two-level" asks for the reference's BLAS / TLAS split (hala_rt_set_build_options: instancing = 2 — primitives that
 * several nodes reference are stored once) instead of one tree over all triangles flattened to world space.
 *
 * --clip N --time T poses the file's skins, morph targets and animated nodes at time T of its clip N before rendering (hala_rt_set_rig,
 * hala_rt_pose_rig); with --shutter T2 the frames blur the clip over [T, T2] instead (hala_rt_key_rig, hala_rt_set_shutter).  Without them
 * an animated file renders in the pose it was saved in.
 *
 * writes out/frame_color.pfm, out/frame_albedo.pfm, out/frame_normal.pfm (the reference's save_images trio). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "halart.h"

static int fail(const char* what) {
  fprintf(stderr, "%s: %s\n", what, hala_last_error_message());
  return 1;
}

int main(int argc, char** argv) {
  long clip = -1;
  float time = 0.0f, shutter = 0.0f;
  int blur = 0, n = 0;
  for (int i = 0; i < argc; ++i) { /* the options leave; the positional arguments stay where they were */
    if (i + 1 < argc && strcmp(argv[i], "--clip") == 0) clip = atol(argv[++i]);
    else if (i + 1 < argc && strcmp(argv[i], "--time") == 0) time = (float)atof(argv[++i]);
    else if (i + 1 < argc && strcmp(argv[i], "--shutter") == 0) { shutter = (float)atof(argv[++i]); blur = 1; }
    else argv[n++] = argv[i];
  }
  argc = n;
  if (argc < 6) {
    fprintf(stderr, "usage: %s scene.gltf out_stem width height spp [envmap [rotation_degrees [two-level]]] [--clip N --time T [--shutter T2]]\n", argv[0]);
    return 2;
  }
  const char* gltf = argv[1];
  const char* stem = argv[2];
  const uint32_t width = (uint32_t)atoi(argv[3]), height = (uint32_t)atoi(argv[4]), spp = (uint32_t)atoi(argv[5]);

  hala_scene* scene = NULL;
  if (hala_scene_load_gltf(gltf, &scene) != 0) return fail("hala_scene_load_gltf");

  hala_rt_renderer* r = NULL;
  if (hala_rt_create("render_gltf", width, height, /*device*/ 0, /*max_depth*/ 8, /*rr_depth*/ 3, /*tonemap*/ 0, /*aces*/ 0,
                     /*simple aces*/ 0, /*max_frames*/ 0, &r) != 0)
    return fail("hala_rt_create");
  if (argc > 6 && hala_rt_set_envmap_file(r, argv[6], argc > 7 ? (float)atof(argv[7]) : 0.0f) != 0) return fail("hala_rt_set_envmap_file");
  if (hala_rt_set_scene(r, hala_scene_get_desc(scene)) != 0) return fail("hala_rt_set_scene");
  if (argc > 8 && strcmp(argv[8], "two-level") == 0) {
    hala_rt_build_options options;
    memset(&options, 0, sizeof options); /* every field 0 = the default */
    options.instancing = 2;
    if (hala_rt_set_build_options(r, &options) != 0) return fail("hala_rt_set_build_options");
  }
  if (hala_rt_commit(r) != 0) return fail("hala_rt_commit");
  {
    hala_bvh_info info;
    if (hala_rt_get_bvh_info(r, &info) != 0) return fail("hala_rt_get_bvh_info");
    printf("triangles %u stored %u instance references %u tree bytes %llu\n", info.triangle_count, info.stored_triangle_count, info.instance_ref_count,
           (unsigned long long)info.tree_bytes);
  }

  if (clip >= 0) { /* the rig: one deformer per skinned or morphed primitive, then the clip's pose or its two shutter keys, then the refit */
    const hala_rig_desc* rig = hala_scene_get_rig(scene);
    if (hala_rt_set_rig(r, rig) != 0) return fail("hala_rt_set_rig");
    if (blur) {
      hala_shutter_params sp;
      hala_shutter_default_params(&sp);
      if (hala_rt_key_rig(r, (uint32_t)clip, time, shutter) != 0) return fail("hala_rt_key_rig");
      if (hala_rt_set_shutter(r, &sp) != 0) return fail("hala_rt_set_shutter");
    } else if (hala_rt_pose_rig(r, (uint32_t)clip, time) != 0) {
      return fail("hala_rt_pose_rig");
    }
    if (hala_rt_refit(r) != 0) return fail("hala_rt_refit");
    printf("clip %ld of %u \"%s\" at %g%s: %u bindings\n", clip, rig->clip_count, rig->clips[clip].name, time, blur ? " (shutter)" : "", rig->binding_count);
  }
  hala_scene_free(scene); /* borrowed until here: the renderer has copied what it needs */

  for (uint32_t k = 0; k < spp; ++k) { /* one sample per pixel per update, like the reference's frame loop */
    if (hala_rt_update(r, 0.0, width, height) != 0) return fail("hala_rt_update");
    if (hala_rt_render(r) != 0) return fail("hala_rt_render");
  }
  if (hala_rt_save_images(r, stem) != 0) return fail("hala_rt_save_images");

  hala_rt_statistics st;
  if (hala_rt_get_statistics(r, &st) != 0) return fail("hala_rt_get_statistics");
  printf("frames %llu rays %llu gpu_ms_total %.3f\n", (unsigned long long)st.total_frames, (unsigned long long)st.rays_total, st.gpu_ms_total);
  hala_rt_destroy(r);
  return 0;
}
