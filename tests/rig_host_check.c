/* Host-memory check of the glTF rig loader and of hala_rig_sample_clip (docs/RENDER_SPEC.md 19), for tests/test_rig.py: built with
 * -fsanitize=address,undefined from this file, tests/rig_host_shim.cpp and the library's host sources (no GPU code), and run as an
 * ordinary process.  Loads every file named on the command line; a file that loads has each of its clips, and its own pose, sampled at
 * times before, inside and after the clip.  Prints one line per file; the sanitizers abort the process on a bad access. */
#include <stdio.h>
#include <stdlib.h>

#include "halart.h"

static int sample(const hala_rig_desc* g, uint32_t clip, float t, float* l, float* w, float* p, double* sum) {
  uint32_t k;
  if (hala_rig_sample_clip(g, clip, t, l, w, p) != 0) return 1;
  for (k = 0; k < g->node_count * 16u; ++k) *sum += l[k];
  for (k = 0; k < g->weight_floats; ++k) *sum += w[k];
  for (k = 0; k < g->palette_floats; ++k) *sum += p[k];
  return 0;
}

int main(int argc, char** argv) {
  int i;
  for (i = 1; i < argc; ++i) {
    hala_scene* s = NULL;
    const hala_rig_desc* g;
    float *l, *w, *p;
    double sum = 0.0;
    uint32_t c, failed = 0, samples = 0;
    if (hala_scene_load_gltf(argv[i], &s) != 0) {
      printf("refused %s: %s\n", argv[i], hala_last_error_message());
      continue;
    }
    g = hala_scene_get_rig(s);
    l = (float*)malloc(sizeof(float) * (g->node_count * 16u + 1u));
    w = (float*)malloc(sizeof(float) * (g->weight_floats + 1u));
    p = (float*)malloc(sizeof(float) * (g->palette_floats + 1u));
    if (!l || !w || !p) return 2;
    failed += (uint32_t)sample(g, HALA_INVALID_INDEX, 0.0f, l, w, p, &sum);
    for (c = 0; c < g->clip_count; ++c) {
      const float a = g->clips[c].time_first, b = g->clips[c].time_last;
      int k;
      for (k = -2; k <= 18; ++k, ++samples) failed += (uint32_t)sample(g, c, a + (b - a) * (float)k / 16.0f, l, w, p, &sum);
    }
    failed += hala_rig_sample_clip(g, g->clip_count, 0.0f, l, w, p) == 0; /* no such clip: refused */
    printf("loaded %s: %u nodes %u skins %u bindings %u clips %u samples %u failed checksum %.6g\n", argv[i], g->node_count, g->skin_count, g->binding_count,
           g->clip_count, samples, failed, sum);
    free(l); free(w); free(p);
    hala_scene_free(s);
  }
  return 0;
}
