// rig.cpp — docs/RENDER_SPEC.md 19: the pose of a hala_rig_desc at a time of one of its clips.  Host code in float64, every result
// rounded to float32 once; no renderer, no GPU and no HIP header, so that a host-only program can be built from this file and the
// loader.  hala_rig_sample_clip is the public face; rt_rig.hip uses rig_sample for hala_rt_pose_rig / hala_rt_key_rig.
#include "rig.h"

#include <cmath>
#include <cstring>

namespace rt {
void set_last_error(const std::string& msg);  // host_util.cpp

namespace {

constexpr uint32_t kMaxRigCount = 1u << 24;  // of nodes, keys and the like: keeps every product of two counts inside size_t

// the description reads nowhere out of bounds: every index it holds is inside the array it names
std::string validate(const hala_rig_desc& g) {
  if (g.node_count > kMaxRigCount || g.skin_count > kMaxRigCount || g.binding_count > kMaxRigCount || g.clip_count > kMaxRigCount) return "a count is out of range";
  if ((g.node_count && !g.nodes) || (g.skin_count && !g.skins) || (g.binding_count && !g.bindings) || (g.clip_count && !g.clips)) return "a table is NULL";
  for (uint32_t n = 0; n < g.node_count; ++n)
    if (g.nodes[n].parent >= (int32_t)n || g.nodes[n].parent < -1) return "node " + std::to_string(n) + " does not come after its parent";
  for (uint32_t k = 0; k < g.skin_count; ++k) {
    const hala_rig_skin& s = g.skins[k];
    if (s.joint_count > kMaxRigCount || (s.joint_count && (!s.joints || !s.inverse_bind_matrices))) return "skin " + std::to_string(k) + " has no joints or no matrices";
    for (uint32_t j = 0; j < s.joint_count; ++j)
      if (s.joints[j] >= g.node_count) return "a joint of skin " + std::to_string(k) + " is out of range";
  }
  for (uint32_t k = 0; k < g.binding_count; ++k) {
    const hala_rig_binding& b = g.bindings[k];
    const std::string where = "the binding of mesh " + std::to_string(b.mesh_index) + " primitive " + std::to_string(b.primitive_index);
    if (b.node >= g.node_count) return "the node of " + where + " is out of range";
    if (b.skin != HALA_INVALID_INDEX) {
      if (b.skin >= g.skin_count) return "the skin of " + where + " is out of range";
      if ((uint64_t)b.palette_first + (uint64_t)g.skins[b.skin].joint_count * 12u > g.palette_floats) return "the palette of " + where + " does not fit a packed pose";
    }
    if (b.target_count > kMaxRigCount || (uint64_t)b.weight_first + b.target_count > g.weight_floats) return "the weights of " + where + " do not fit a packed pose";
    if (b.target_count && !b.default_weights) return where + " has no default weights";
  }
  for (uint32_t c = 0; c < g.clip_count; ++c) {
    const hala_rig_clip& clip = g.clips[c];
    const std::string which = "clip " + std::to_string(c);
    if (clip.sampler_count > kMaxRigCount || clip.channel_count > kMaxRigCount || (clip.sampler_count && !clip.samplers) || (clip.channel_count && !clip.channels))
      return which + " has a table that is NULL";
    for (uint32_t k = 0; k < clip.sampler_count; ++k) {
      const hala_rig_sampler& s = clip.samplers[k];
      if (!s.key_count || s.key_count > kMaxRigCount || !s.width || s.width > kMaxRigCount || s.interpolation > HALA_RIG_CUBICSPLINE || !s.times || !s.values)
        return "a sampler of " + which + " is malformed";
    }
    for (uint32_t k = 0; k < clip.channel_count; ++k) {
      const hala_rig_channel& ch = clip.channels[k];
      if (ch.sampler >= clip.sampler_count || ch.node >= g.node_count || ch.path > HALA_RIG_WEIGHTS) return "a channel of " + which + " is out of range";
      if (g.nodes[ch.node].is_matrix) return "a channel of " + which + " targets a node given as a matrix";
      const uint32_t w = clip.samplers[ch.sampler].width;
      if (ch.path == HALA_RIG_WEIGHTS) {
        for (uint32_t b = 0; b < g.binding_count; ++b)
          if (g.bindings[b].node == ch.node && g.bindings[b].target_count != w) return "a weights channel of " + which + " differs in width from its mesh's target count";
      } else if (w != (ch.path == HALA_RIG_ROTATION ? 4u : 3u)) {
        return "a channel of " + which + " reads a sampler of the wrong width";
      }
    }
  }
  return "";
}

void normalise4(double* q) {
  const double len = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int c = 0; c < 4; ++c) q[c] = q[c] / len;
}

// RENDER_SPEC 19 "Key lookup" and "Interpolation": the value of sampler `s` at `t` -> out[width]
void sample(const hala_rig_sampler& s, double t, bool rotation, double* out) {
  const uint32_t n = s.key_count, w = s.width;
  const bool cubic = s.interpolation == HALA_RIG_CUBICSPLINE;
  const size_t stride = cubic ? 3u * (size_t)w : w, value = cubic ? w : 0u;  // a CUBICSPLINE key: in-tangent, value, out-tangent
  auto key = [&](uint32_t k) { return s.values + (size_t)k * stride + value; };
  if (n == 1 || !(t > (double)s.times[0])) { for (uint32_t c = 0; c < w; ++c) out[c] = key(0)[c]; return; }
  if (!(t < (double)s.times[n - 1])) { for (uint32_t c = 0; c < w; ++c) out[c] = key(n - 1)[c]; return; }
  uint32_t lo = 0, hi = n - 1;  // times[lo] <= t < times[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((double)s.times[mid] <= t) lo = mid; else hi = mid;
  }
  const double t0 = s.times[lo], t1 = s.times[lo + 1], dt = t1 - t0, u = (t - t0) / dt;
  const float* a = key(lo);
  const float* b = key(lo + 1);
  if (s.interpolation == HALA_RIG_STEP) {
    for (uint32_t c = 0; c < w; ++c) out[c] = a[c];
  } else if (cubic) {
    const float* out_tangent = a + w;       // b_k
    const float* in_tangent = b - w;        // a_{k+1}
    const double u2 = u * u, u3 = u2 * u;
    for (uint32_t c = 0; c < w; ++c)
      out[c] = (2.0 * u3 - 3.0 * u2 + 1.0) * (double)a[c] + (u3 - 2.0 * u2 + u) * (dt * (double)out_tangent[c]) + (-2.0 * u3 + 3.0 * u2) * (double)b[c] +
               (u3 - u2) * (dt * (double)in_tangent[c]);
    if (rotation) normalise4(out);
  } else if (rotation) {  // the shorter arc
    double q1[4] = {b[0], b[1], b[2], b[3]};
    double d = (double)a[0] * q1[0] + (double)a[1] * q1[1] + (double)a[2] * q1[2] + (double)a[3] * q1[3];
    if (d < 0.0) { d = -d; for (double& x : q1) x = -x; }
    if (d > 0.9995) {
      for (int c = 0; c < 4; ++c) out[c] = (double)a[c] + u * (q1[c] - (double)a[c]);
      normalise4(out);
    } else {
      const double theta = std::acos(d), sn = std::sin(theta), wa = std::sin((1.0 - u) * theta) / sn, wb = std::sin(u * theta) / sn;
      for (int c = 0; c < 4; ++c) out[c] = wa * (double)a[c] + wb * q1[c];
    }
  } else {
    for (uint32_t c = 0; c < w; ++c) out[c] = (double)a[c] + u * ((double)b[c] - (double)a[c]);
  }
}

// T * R * S, column-major, rounded once (gltf_loader.cpp's node_matrix on sampled components)
void compose(const double* t, const double* q, const double* s, float m[16]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double r[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                          {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                          {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
  for (int c = 0; c < 3; ++c) {
    for (int rr = 0; rr < 3; ++rr) m[4 * c + rr] = (float)(r[rr][c] * s[c]);
    m[4 * c + 3] = 0.0f;
  }
  m[12] = (float)t[0]; m[13] = (float)t[1]; m[14] = (float)t[2]; m[15] = 1.0f;
}

struct M4 { double m[16]; };  // column-major
M4 mul(const M4& a, const M4& b) {
  M4 o;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      double acc = 0.0;
      for (int k = 0; k < 4; ++k) acc += a.m[4 * k + r] * b.m[4 * c + k];
      o.m[4 * c + r] = acc;
    }
  return o;
}
// Gauss-Jordan with partial pivoting; false: singular (a pivot of 0) or not finite
bool invert(const M4& a, M4* out) {
  double w[4][8];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) { w[r][c] = a.m[4 * c + r]; w[r][4 + c] = r == c ? 1.0 : 0.0; }
  for (int col = 0; col < 4; ++col) {
    int piv = col;
    for (int r = col + 1; r < 4; ++r) if (std::fabs(w[r][col]) > std::fabs(w[piv][col])) piv = r;
    if (!(std::fabs(w[piv][col]) > 0.0) || !std::isfinite(w[piv][col])) return false;
    if (piv != col) for (int c = 0; c < 8; ++c) std::swap(w[piv][c], w[col][c]);
    const double d = w[col][col];
    for (int c = 0; c < 8; ++c) w[col][c] /= d;
    for (int r = 0; r < 4; ++r) {
      if (r == col) continue;
      const double f = w[r][col];
      if (f != 0.0) for (int c = 0; c < 8; ++c) w[r][c] -= f * w[col][c];
    }
  }
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      if (!std::isfinite(w[r][4 + c])) return false;
      out->m[4 * c + r] = w[r][4 + c];
    }
  return true;
}

}  // namespace

std::string rig_validate(const hala_rig_desc* rig) {
  if (!rig) return "The rig description is NULL.";
  const std::string bad = validate(*rig);
  return bad.empty() ? "" : "The rig description is malformed: " + bad + ".";
}

void RigCopy::assign(const hala_rig_desc& g) {
  clear();
  auto keep_f32 = [this](const float* p, size_t n) { f32s.emplace_back(p, p + n); return (const float*)f32s.back().data(); };
  // (the inner vectors are moved, never copied, when the outer ones grow: the pointers taken here stay good)
  nodes.assign(g.nodes, g.nodes + g.node_count);
  if (g.node_of_gltf) node_of_gltf.assign(g.node_of_gltf, g.node_of_gltf + g.gltf_node_count);
  for (uint32_t k = 0; k < g.skin_count; ++k) {
    hala_rig_skin s = g.skins[k];
    u32s.emplace_back(s.joints, s.joints + s.joint_count);
    s.joints = u32s.back().data();
    s.inverse_bind_matrices = keep_f32(s.inverse_bind_matrices, (size_t)s.joint_count * 16u);
    skins.push_back(s);
  }
  for (uint32_t k = 0; k < g.binding_count; ++k) {
    hala_rig_binding b = g.bindings[k];
    b.joints = nullptr; b.weights = nullptr;
    b.target_position_deltas = b.target_normal_deltas = b.target_tangent_deltas = nullptr;
    b.default_weights = b.target_count ? keep_f32(b.default_weights, b.target_count) : nullptr;
    bindings.push_back(b);
  }
  for (uint32_t c = 0; c < g.clip_count; ++c) {
    hala_rig_clip cl = g.clips[c];
    names.emplace_back(cl.name ? cl.name : "");
    samplers.emplace_back(cl.samplers, cl.samplers + cl.sampler_count);
    channels.emplace_back(cl.channels, cl.channels + cl.channel_count);
    for (hala_rig_sampler& s : samplers.back()) {
      const size_t n = (size_t)s.key_count * s.width * (s.interpolation == HALA_RIG_CUBICSPLINE ? 3u : 1u);
      s.times = keep_f32(s.times, s.key_count);
      s.values = keep_f32(s.values, n);
    }
    clips.push_back(cl);
  }
  for (size_t c = 0; c < clips.size(); ++c) {  // (std::string may keep short names inside itself: taken once `names` is complete)
    clips[c].name = names[c].c_str();
    clips[c].samplers = samplers[c].data(); clips[c].channels = channels[c].data();
  }
  desc = g;
  desc.nodes = nodes.data(); desc.node_of_gltf = node_of_gltf.empty() ? nullptr : node_of_gltf.data();
  desc.gltf_node_count = (uint32_t)node_of_gltf.size();
  desc.skins = skins.data(); desc.bindings = bindings.data(); desc.clips = clips.data();
}

std::string rig_sample(const hala_rig_desc* rig, uint32_t clip, float time, RigPose* out, bool validated) {
  if (!validated) {
    const std::string bad = rig_validate(rig);
    if (!bad.empty()) return bad;
  }
  const hala_rig_desc& g = *rig;
  if (clip != HALA_INVALID_INDEX && clip >= g.clip_count) return "The clip does not exist.";
  if (!std::isfinite(time)) return "The time is not finite.";
  const double t = time;
  out->clip = clip; out->time = time;
  out->locals.resize((size_t)g.node_count * 16u);
  out->weights.assign(g.weight_floats, 0.0f);
  out->palettes.assign(g.palette_floats, 0.0f);
  out->touched.assign(g.node_count, 0);
  // nodes: the loaded bytes, then T * R * S of the nodes the clip touches
  for (uint32_t n = 0; n < g.node_count; ++n) memcpy(&out->locals[(size_t)n * 16u], g.nodes[n].local_transform, 64);
  for (uint32_t b = 0; b < g.binding_count; ++b)
    for (uint32_t k = 0; k < g.bindings[b].target_count; ++k) out->weights[g.bindings[b].weight_first + k] = g.bindings[b].default_weights[k];
  if (clip == HALA_INVALID_INDEX) {  // the file's own pose, on every node any clip touches
    for (uint32_t c = 0; c < g.clip_count; ++c)
      for (uint32_t k = 0; k < g.clips[c].channel_count; ++k)
        if (g.clips[c].channels[k].path != HALA_RIG_WEIGHTS) out->touched[g.clips[c].channels[k].node] = 1;
  } else {
    const hala_rig_clip& cl = g.clips[clip];
    std::vector<double> trs((size_t)g.node_count * 10u);
    for (uint32_t n = 0; n < g.node_count; ++n) {
      double* p = &trs[(size_t)n * 10u];
      for (int c = 0; c < 3; ++c) { p[c] = g.nodes[n].translation[c]; p[7 + c] = g.nodes[n].scale[c]; }
      for (int c = 0; c < 4; ++c) p[3 + c] = g.nodes[n].rotation[c];
    }
    std::vector<double> w;
    for (uint32_t k = 0; k < cl.channel_count; ++k) {
      const hala_rig_channel& ch = cl.channels[k];
      const hala_rig_sampler& s = cl.samplers[ch.sampler];
      if (ch.path == HALA_RIG_WEIGHTS) {
        w.resize(s.width);
        sample(s, t, false, w.data());
        for (uint32_t b = 0; b < g.binding_count; ++b)
          if (g.bindings[b].node == ch.node)
            for (uint32_t i = 0; i < s.width; ++i) out->weights[g.bindings[b].weight_first + i] = (float)w[i];
        continue;
      }
      double* p = &trs[(size_t)ch.node * 10u];
      sample(s, t, ch.path == HALA_RIG_ROTATION, ch.path == HALA_RIG_TRANSLATION ? p : ch.path == HALA_RIG_ROTATION ? p + 3 : p + 7);
      out->touched[ch.node] = 1;
    }
    for (uint32_t n = 0; n < g.node_count; ++n)
      if (out->touched[n]) { const double* p = &trs[(size_t)n * 10u]; compose(p, p + 3, p + 7, &out->locals[(size_t)n * 16u]); }
  }
  for (float v : out->locals) if (!std::isfinite(v)) return "A posed node transform is not finite.";
  for (float v : out->weights) if (!std::isfinite(v)) return "A posed morph weight is not finite.";
  // worlds: the float64 product of the float32 locals down the hierarchy (parents come first)
  std::vector<M4> world(g.node_count);
  for (uint32_t n = 0; n < g.node_count; ++n) {
    M4 l;
    for (int i = 0; i < 16; ++i) l.m[i] = out->locals[(size_t)n * 16u + i];
    world[n] = g.nodes[n].parent < 0 ? l : mul(world[g.nodes[n].parent], l);
  }
  for (uint32_t b = 0; b < g.binding_count; ++b) {
    const hala_rig_binding& bd = g.bindings[b];
    if (bd.skin == HALA_INVALID_INDEX) continue;
    const hala_rig_skin& sk = g.skins[bd.skin];
    M4 inv;
    if (!invert(world[bd.node], &inv))
      return "The world transform of the node of mesh " + std::to_string(bd.mesh_index) + " is singular: its skin cannot be posed.";
    for (uint32_t j = 0; j < sk.joint_count; ++j) {
      M4 ibm;
      for (int i = 0; i < 16; ++i) ibm.m[i] = sk.inverse_bind_matrices[(size_t)j * 16u + i];
      const M4 m = mul(mul(inv, world[sk.joints[j]]), ibm);
      float* dst = &out->palettes[bd.palette_first + (size_t)j * 12u];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
          dst[4 * r + c] = (float)m.m[4 * c + r];
          if (!std::isfinite(dst[4 * r + c])) return "A posed joint matrix is not finite.";
        }
    }
  }
  return "";
}

}  // namespace rt

extern "C" int hala_rig_sample_clip(const hala_rig_desc* rig, uint32_t clip, float time, float* locals, float* weights, float* palettes) {
  rt::RigPose pose;
  const std::string e = rt::rig_sample(rig, clip, time, &pose);
  if (!e.empty()) { rt::set_last_error(e); return HALA_ERR; }
  if (locals && !pose.locals.empty()) memcpy(locals, pose.locals.data(), pose.locals.size() * 4u);
  if (weights && !pose.weights.empty()) memcpy(weights, pose.weights.data(), pose.weights.size() * 4u);
  if (palettes && !pose.palettes.empty()) memcpy(palettes, pose.palettes.data(), pose.palettes.size() * 4u);
  return HALA_OK;
}
