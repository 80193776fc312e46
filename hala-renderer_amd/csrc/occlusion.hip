// occlusion.hip — occlusion batches (RENDER_SPEC 4.10): for every sample (a point with a normal) of a batch, N cosine-distributed any-hit
// rays over the hemisphere of the normal, reduced to the share of unoccluded rays and their bent normal.  Two kernels.
// k_trace_occlusion is the any-hit batch kernel of trace_closest.hip with another ray source: the persistent loop of trace_loop.h
// (persistent_trace<true, false, ...>, unchanged: a new Source type only adds instantiations) over the queue [0, count * N), whose
// entry i * N + j is ray j of sample i, generated in the lane that traces it — no ray queue in memory, as for the camera rays of a
// frame (CameraSource).  An occluded ray sets its bit of the sample's mask words; OR commutes, so the masks do not depend on the order
// the rays finish in.  k_occlusion_resolve then runs one lane per sample: it regenerates the directions of the clear bits in ascending j
// (occ_direction, the same function: the same bits) and writes the 16-B record.
// The listed forms (k_trace_occlusion_listed, k_occlusion_resolve_listed) do the same for the samples a device-built list names, its
// length read on the device: the occlusion pass of a bake atlas (RENDER_SPEC 4.12), which skips the texels nothing covers.
// Not one of the flag-dispatched families of variants.h: launched like the multi-hit kernel (tree_form, with_flags), with the launch
// shape of an any-hit batch (lc.persistent_blocks, lc.smem: the same launch bounds and the same LDS as k_trace_batch).
#include "trace_loop.h"
#include "variants.h"

namespace rt {

// What a sample gives all of its rays: the unit normal with its basis (RENDER_SPEC 2.4) and the common origin
struct OccFrame {
  f3 n, t, b, o;
};
// RENDER_SPEC 4.10, validity: nn > 0, nn < +inf, point and bias finite (a NaN fails every comparison).  One expression for both kernels.
RT_DI bool occ_valid(float4 pb, float4 nr, float* nn_out) {
  constexpr float kInf = __builtin_huge_valf();
  const float nn = dot3(mk3(nr.x, nr.y, nr.z), mk3(nr.x, nr.y, nr.z));
  *nn_out = nn;
  return nn > 0.0f && nn < kInf && fabsf(pb.x) < kInf && fabsf(pb.y) < kInf && fabsf(pb.z) < kInf && fabsf(pb.w) < kInf;
}
RT_DI OccFrame occ_frame(float4 pb, float4 nr, float nn) {
  OccFrame f;
  f.n = mk3(nr.x, nr.y, nr.z) * rcp_rn(sqrt_rn(nn));
  onb(f.n, &f.t, &f.b);
  f.o = madd3(f.n, pb.w, mk3(pb.x, pb.y, pb.z));
  return f;
}
// the stream of sample i: RENDER_SPEC 2.3 with pixel_id = i and frame_index = seed; seed_key = pcg(seed * 0x9E3779B9 + 0x85EBCA6B)
RT_DI uint32_t occ_stream(uint32_t i, uint32_t seed_key) { return pcg_hash(i + seed_key); }
// direction j of a sample: draws 2j and 2j + 1 of its stream by random access, cosine-distributed around n, not normalised again
RT_DI f3 occ_direction(const OccFrame& f, uint32_t s, uint32_t j) {
  const float u1 = (float)(pcg_hash(s + 2u * j) >> 8) * (1.0f / 16777216.0f);
  const float u2 = (float)(pcg_hash(s + 2u * j + 1u) >> 8) * (1.0f / 16777216.0f);
  return to_world(cosine_hemisphere(u1, u2), f.t, f.b, f.n);
}

// LISTED (the bake atlases of RENDER_SPEC 4.12): queue entry c * rays + j is ray j of sample list[c].  Sample, stream and any-hit key
// are those of sample i = list[c] — the ray is the one the unlisted queue holds at i * rays + j, bit for bit; only the mask words are
// the list position's (masks + c * words), so that the runs done() reasons on are still runs of queue entries.  A template flag: the
// unlisted kernels keep their code.
template <bool LISTED>
struct OcclusionSourceT {
  struct Payload {};
  const SceneView& sv;
  const float4* samples;  // 32 B each: (point, bias), (normal, reach)
  uint32_t* masks;        // words per sample, zeroed by the caller
  uint32_t rays, words, seed_key;
  const uint32_t* list = nullptr;  // LISTED: the sample of each list position
  RT_DI bool load(uint32_t idx, f3* o, f3* d, float* tmin, float* tmax, uint32_t* key, Payload*) const {
    const uint32_t c = idx / rays, j = idx - c * rays;
    uint32_t i = c, ray = idx;
    if constexpr (LISTED) { i = list[c]; ray = i * rays + j; }  // (< 2^32: i < the map's texels, whose rays the caller has checked)
    const float4 pb = samples[(size_t)i * 2], nr = samples[(size_t)i * 2 + 1];
    float nn;
    if (!occ_valid(pb, nr, &nn)) return false;  // traces nothing: its words stay 0, the resolve kernel writes the invalid record
    const OccFrame f = occ_frame(pb, nr, nn);
    *o = f.o; *d = occ_direction(f, occ_stream(i, seed_key), j);
    *tmin = 0.0f; *tmax = nr.w;
    *key = pcg_hash(ray ^ kAnyKeyBatch);  // RENDER_SPEC 7.1d: the key of ray i * N + j of a batch
    rebase_ray(sv, *o, *d, *tmin, *tmax);  // RENDER_SPEC 4.2; an any-hit ray reports no t, so the distance moved is not kept
    return true;
  }
  // Called by the lanes whose rays finished since the wave's last refill, together.  Where their queue entries run with the lane index
  // (entry = lane + a constant: the whole-wave batches of the staged kernels, and every refill that fills a run of lanes), the lanes of
  // one mask word are a run of lanes and the word's bits are the wave's ballot of "occluded", shifted: the first of them issues ONE
  // atomic for all.  The others issue one per lane.  (32 lanes OR-ing one word are 32 atomics on one address, served one after the
  // other: on the Cornell box they cost 0.08 of a batch's 0.22 ms at N = 64)  No value comes back: no lane waits for it.
  RT_DI void done(uint32_t idx, const Trav& t, const Payload&) const {
    const bool occluded = t.best.prim != kAbsent;  // an unoccluded ray's bit stays 0
    const uint32_t i = idx / rays, j = idx - i * rays, lane = lane_id();
    uint32_t* word = masks + (size_t)i * words + (j >> 5);
    const unsigned long long active = __ballot(true), hit = __ballot(occluded);
    const uint32_t rel = idx - lane;  // (wraps; compared only)
    if (__ballot(rel == lane0_u32(rel)) != active) {  // lane0_u32: the first active lane's value
      if (occluded) atomicOr(word, 1u << (j & 31u));
      return;
    }
    const int first = (int)lane - (int)(j & 31u);  // the lane that holds, or would hold, the word's bit 0: -31 .. 63
    const uint32_t from = first > 0 ? (uint32_t)first : 0u;
    const uint32_t in_word = min(32u, rays - (j & ~31u));  // behind them the next sample's rays follow, which have another word
    const uint32_t bits = (uint32_t)(first >= 0 ? hit >> first : hit << -first) & (in_word == 32u ? ~0u : (1u << in_word) - 1u);
    const unsigned long long before = active & ((1ull << lane) - 1ull) & ~((1ull << from) - 1ull);  // active lanes of this word below this one
    if (before == 0ull && bits != 0u) atomicOr(word, bits);
  }
};
typedef OcclusionSourceT<false> OcclusionSource;

// (The two-level form with translucent materials carries the instance transitions next to the texture fetch of 7.1d: with the ray
// generation inlined into its refill it spilled 9 registers to scratch at the 96 of 5 waves per SIMD, so it is built for 4 like the
// staged form.  The grid stays lc.persistent_blocks: the loop has no grid-wide wait, a workgroup that starts late finds the queue dry.)
template <bool STAGED, bool ALPHA, bool INST>
__global__ void __launch_bounds__(kTraverseThreads, (STAGED || (ALPHA && INST)) ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_trace_occlusion(SceneView sv, const float4* __restrict__ samples, uint32_t* __restrict__ masks, uint32_t n, uint32_t rays, uint32_t words,
                  uint32_t seed_key, WorkCounters* __restrict__ work, uint2* __restrict__ spill_base, uint32_t refill) {
  const TraverseLds lds = stage_bvh<STAGED, INST>(sv, g_smem);
  uint2* spill = lane_spill(spill_base);
  StepCounters sc;
  OcclusionSource src{sv, samples, masks, rays, words, seed_key};
  persistent_trace<true, false, STAGED, ALPHA, INST>(sv, lds, spill, work, n, refill, src, sc);
}

// The listed kernel: n = *count * rays is read on the device (no word to the host), as the shadow kernels read their queue sizes.  Bakes
// are refused on two-level trees: no INST form.
template <bool STAGED, bool ALPHA>
__global__ void __launch_bounds__(kTraverseThreads, STAGED ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_trace_occlusion_listed(SceneView sv, const float4* __restrict__ samples, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                         uint32_t* __restrict__ masks, uint32_t rays, uint32_t words, uint32_t seed_key, WorkCounters* __restrict__ work,
                         uint2* __restrict__ spill_base, uint32_t refill) {
  const TraverseLds lds = stage_bvh<STAGED, false>(sv, g_smem);
  uint2* spill = lane_spill(spill_base);
  StepCounters sc;
  OcclusionSourceT<true> src{sv, samples, masks, rays, words, seed_key, list};
  persistent_trace<true, false, STAGED, ALPHA, false>(sv, lds, spill, work, *count * rays, refill, src, sc);
}

// The record of sample i from its mask words m: visibility = clear / N, bent = the normalised sum of the unoccluded directions in ascending j
RT_DI void occ_resolve(const float4* __restrict__ samples, const uint32_t* __restrict__ m, float4* __restrict__ out, uint32_t i, uint32_t rays,
                       uint32_t words, uint32_t seed_key) {
  const float4 pb = samples[(size_t)i * 2], nr = samples[(size_t)i * 2 + 1];
  float nn;
  if (!occ_valid(pb, nr, &nn)) { out[i] = make_float4(-1.0f, 0.0f, 0.0f, 0.0f); return; }
  const OccFrame f = occ_frame(pb, nr, nn);
  const uint32_t s = occ_stream(i, seed_key);
  uint32_t clear = 0u;
  f3 sum = splat3(0.0f);
  for (uint32_t w = 0; w < words; ++w) {
    const uint32_t in_word = min(32u, rays - w * 32u);
    uint32_t open = ~m[w] & (in_word == 32u ? ~0u : (1u << in_word) - 1u);
    clear += (uint32_t)__popc(open);
    while (open) {
      const uint32_t k = (uint32_t)__ffs((int)open) - 1u;
      open &= open - 1u;
      sum = sum + occ_direction(f, s, w * 32u + k);
    }
  }
  const float ss = dot3(sum, sum);
  const f3 bent = ss > 0.0f ? sum * rcp_rn(sqrt_rn(ss)) : splat3(0.0f);
  out[i] = make_float4((float)clear / (float)rays, bent.x, bent.y, bent.z);
}
// One lane per sample
__global__ void __launch_bounds__(256) k_occlusion_resolve(const float4* __restrict__ samples, const uint32_t* __restrict__ masks, float4* __restrict__ out,
                                                           uint32_t count, uint32_t rays, uint32_t words, uint32_t seed_key) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  occ_resolve(samples, masks + (size_t)i * words, out, i, rays, words, seed_key);
}
// One lane per list entry (the grid covers the largest list there can be): the record of sample list[c] from the words of position c
__global__ void __launch_bounds__(256) k_occlusion_resolve_listed(const float4* __restrict__ samples, const uint32_t* __restrict__ list,
                                                                  const uint32_t* __restrict__ count, const uint32_t* __restrict__ masks,
                                                                  float4* __restrict__ out, uint32_t rays, uint32_t words, uint32_t seed_key) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= *count) return;
  occ_resolve(samples, masks + (size_t)c * words, out, list[c], rays, words, seed_key);
}

// pcg (RENDER_SPEC 2.3) of seed * 0x9E3779B9 + 0x85EBCA6B, on the host: uint32 arithmetic, the same bits
static uint32_t occ_seed_key(uint32_t seed) {
  uint32_t state = seed * 0x9E3779B9u + 0x85EBCA6Bu;
  state = state * 747796405u + 2891336453u;
  const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
  return (word >> 22u) ^ word;
}
void launch_trace_occlusion(const LaunchCfg& lc, const SceneView& sv, const hala_occlusion_sample* samples, hala_occlusion* out, uint32_t* masks,
                            uint32_t count, uint32_t rays, uint32_t seed, WorkCounters* work, hipStream_t s) {
  SceneView sva = sv;
  sva.tris = sv.tris_any;  // RENDER_SPEC 7.1d: what every any-hit launch traverses
  const TreeForm tree = tree_form(sv);
  const uint32_t words = (rays + 31u) / 32u, n = count * rays;  // (count * rays < 2^32: the caller's check)
  const uint32_t seed_key = occ_seed_key(seed);
  const float4* sp = reinterpret_cast<const float4*>(samples);
  with_flags([&](auto STAGED, auto ALPHA, auto INST) {
    if constexpr (!(STAGED && INST))
      hipLaunchKernelGGL((k_trace_occlusion<STAGED, ALPHA, INST>), dim3(lc.persistent_blocks), dim3(kTraverseThreads), lc.smem, s, sva, sp, masks, n, rays, words,
                         seed_key, work, lc.spill, lc.refill);
  }, tree == TreeForm::Staged, sv.any_translucent != 0u, tree == TreeForm::TwoLevel);
  hipLaunchKernelGGL(k_occlusion_resolve, dim3(blocks_for(count, 256)), dim3(256), 0, s, sp, masks, reinterpret_cast<float4*>(out), count, rays, words, seed_key);
}
void launch_trace_occlusion_listed(const LaunchCfg& lc, const SceneView& sv, const hala_occlusion_sample* samples, const uint32_t* list, const uint32_t* count,
                                   uint32_t max_count, hala_occlusion* out, uint32_t* masks, uint32_t rays, uint32_t seed, WorkCounters* work, hipStream_t s) {
  SceneView sva = sv;
  sva.tris = sv.tris_any;
  const uint32_t words = (rays + 31u) / 32u, seed_key = occ_seed_key(seed);
  const float4* sp = reinterpret_cast<const float4*>(samples);
  with_flags([&](auto STAGED, auto ALPHA) {
    hipLaunchKernelGGL((k_trace_occlusion_listed<STAGED, ALPHA>), dim3(lc.persistent_blocks), dim3(kTraverseThreads), lc.smem, s, sva, sp, list, count, masks, rays,
                       words, seed_key, work, lc.spill, lc.refill);
  }, tree_form(sv) == TreeForm::Staged, sv.any_translucent != 0u);
  hipLaunchKernelGGL(k_occlusion_resolve_listed, dim3(blocks_for(max_count, 256)), dim3(256), 0, s, sp, list, count, masks, reinterpret_cast<float4*>(out), rays,
                     words, seed_key);
}

}  // namespace rt
