// shade.hip — what the wavefront path tracer does between two traversals (trace_closest.hip has the frame's kernel sequence): the kind
// sort of a bounce's queue, and closest-hit + miss + NEE + BSDF sampling for one bounce with the ballot compaction of what it emits.
#include "shading.h"
#include "variants.h"

namespace rt {
// Block-level compaction of up to two predicates at once: one atomic per workgroup and counter instead of one per
// wave (a single counter word takes ~88 atomics/us; a 2 M-path launch of 64-lane waves would need 32 K of them).
// All threads of the block must call it.  Returns this lane's output index for each predicate.
// Workgroup size of k_shade: 512 for the SIMPLE variant, 256 for the generic one (configs[3]: 512 / 256 threads = 3.33 / 3.21 ms of shade
// per frame — fewer waves behind every barrier of the kind sort and of the compaction — while the Cornell box loses 25 % at 256:
// profiles/r02_experiments.txt).  kShadeThreads sizes the shared arrays.
#ifndef RT_SHADE_THREADS
#define RT_SHADE_THREADS 512
#endif
#ifndef RT_SHADE_THREADS_GENERIC
#define RT_SHADE_THREADS_GENERIC 256
#endif
constexpr int kShadeThreads = RT_SHADE_THREADS;
constexpr int kShadeThreadsGeneric = RT_SHADE_THREADS_GENERIC < RT_SHADE_THREADS ? RT_SHADE_THREADS_GENERIC : RT_SHADE_THREADS;
struct BlockCompact {
  uint32_t cnt[3][kShadeThreads / 64];
  uint32_t base[3];
};
// Three predicates at once (surviving path, light connection, environment connection); counters[k] receives the
// block total of predicate k; shadow_total (64-bit) receives the number of connections (predicates 1 + 2).
RT_DI void block_compact3(BlockCompact& sm, const bool keep[3], uint32_t* const counters[3], unsigned long long* shadow_total,
                          uint32_t out[3]) {
  unsigned long long m[3];
  const uint32_t w = threadIdx.x >> 6, l = lane_id();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    m[k] = __ballot(keep[k]);
    if (l == 0u) sm.cnt[k][w] = (uint32_t)__popcll(m[k]);
  }
  __syncthreads();
  const uint32_t nw = blockDim.x >> 6;
  if (threadIdx.x < 3u) {
    uint32_t total = 0;
    for (uint32_t j = 0; j < nw; ++j) total += sm.cnt[threadIdx.x][j];
    sm.base[threadIdx.x] = total ? atomicAdd(counters[threadIdx.x], total) : 0u;
  } else if (threadIdx.x == 64u) {
    uint32_t total = 0;
    for (uint32_t j = 0; j < nw; ++j) total += sm.cnt[1][j] + sm.cnt[2][j];
    if (total) atomicAdd(shadow_total, (unsigned long long)total);
  }
  __syncthreads();
  const unsigned long long below = (1ull << l) - 1ull;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    uint32_t p = sm.base[k];
    for (uint32_t j = 0; j < w; ++j) p += sm.cnt[k][j];
    out[k] = p + (uint32_t)__popcll(m[k] & below);
  }
}
// ---------------------------------------------------------------------------------------------------------
// shade: closest-hit + miss + light/env NEE + BSDF sampling + Russian roulette for one bounce (RENDER_SPEC §6)
// ---------------------------------------------------------------------------------------------------------
// PRIMARY (depth 0): queue entry i IS path slot i, its ray is re-evaluated from the camera instead of being read, and
// the path state starts from its constants (throughput 1, radiance 0) — this kernel initialises every per-path record.
#ifndef RT_SHADE_WAVES
#define RT_SHADE_WAVES 4
#endif
#ifndef RT_SHADE_WAVES_SIMPLE
#define RT_SHADE_WAVES_SIMPLE 6  // 80 VGPRs, no scratch (8 waves: 32-44 B of scratch per lane and slower; profiles/r02_experiments.txt)
#endif
// SCATTER: some material holds a scattering medium (§7.1f): only then does the kernel carry the free-flight / phase-function code
// Bounce launches of scenes whose materials span several shading kinds: the paths of a WINDOW of kSortWindow consecutive queue entries
// are shaded in the order of their shading kind, so that a wave runs one flavour of the BSDF code.  k_shade_sort writes the order (a
// permutation of each window: counting sort through LDS; the kind sits in the low bits of the hit record's prim word, so the sort reads
// nothing but the hit queue), k_shade reads it.  Sorting inside each 256-path workgroup of k_shade left 36 of 64 lanes per vector
// instruction — a partial wave at every kind boundary of every 4-wave block (profiles/r02_w_pmc_config4.txt); a window of 4096 has the
// same boundaries per 64 waves.  Which lane shades which path is not observable: every output is indexed by path slot or comes out
// of the block compaction.
#ifndef RT_SORT_ROUNDS
#define RT_SORT_ROUNDS 4
#endif
#ifndef RT_SORT_THREADS
#define RT_SORT_THREADS 1024  // a window is one workgroup of the sort kernel: 16 waves x 4 entries per lane (256 x 16: 27 us per launch instead of ~12)
#endif
constexpr uint32_t kSortThreads = RT_SORT_THREADS, kSortRounds = RT_SORT_ROUNDS, kSortWindow = kSortThreads * kSortRounds;
static_assert(kSortWindow <= 65536, "window-relative positions are 16-bit in LDS");
__global__ void __launch_bounds__(kSortThreads) k_shade_sort(Queues q, const Control* __restrict__ ctl, uint32_t depth) {
  const uint32_t n = ctl->sizes.n_active[depth];
  const uint32_t base = blockIdx.x * kSortWindow;
  if (base >= n) return;
  const uint32_t live = min(kSortWindow, n - base);
  constexpr uint32_t kWaves = kSortThreads / 64, kCells = kShadeKinds * kSortRounds * kWaves;
  __shared__ uint32_t s_bin[kCells];  // [kind][round][wave]: entries of that kind among the 64 the wave looked at in that round
  const uint32_t w = threadIdx.x >> 6, l = lane_id();
  uint32_t kr[kSortRounds];  // kind | rank << 4 of this thread's entry of round j
#pragma unroll
  for (uint32_t j = 0; j < kSortRounds; ++j) {
    const uint32_t e = j * kSortThreads + threadIdx.x;
    uint32_t kind = kShadeKinds - 1u;  // no path
    if (e < live) {
      const uint32_t pw = reinterpret_cast<const uint32_t*>(q.hits + base + e)[3];
      kind = pw == kAbsent ? kShadeKindMiss : (pw & 7u);
    }
    uint32_t rank = 0;
#pragma unroll
    for (uint32_t b = 0; b < kShadeKinds; ++b) {
      const unsigned long long m = __ballot(kind == b);
      if (kind == b) rank = mbcnt64(m);
      if (l == 0u) s_bin[(b * kSortRounds + j) * kWaves + w] = (uint32_t)__popcll(m);
    }
    kr[j] = kind | (rank << 4);
  }
  __syncthreads();
  if (w == 0u) {  // exclusive prefix over the cells in (kind, round, wave) order, by one wave: each lane folds a run of cells, the runs are scanned with shuffles
    constexpr uint32_t kRun = (kCells + 63u) / 64u;
    uint32_t v[kRun], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRun; ++k) { const uint32_t c = l * kRun + k; v[k] = c < kCells ? s_bin[c] : 0u; sum += v[k]; }
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, off); if (l >= (uint32_t)off) incl += o; }
    uint32_t run = incl - sum;
#pragma unroll
    for (uint32_t k = 0; k < kRun; ++k) { const uint32_t c = l * kRun + k; if (c < kCells) s_bin[c] = run; run += v[k]; }
  }
  __syncthreads();
  // "no path" entries (beyond the queue's end) sort last: positions >= live, never read
#pragma unroll
  for (uint32_t j = 0; j < kSortRounds; ++j) {
    const uint32_t e = j * kSortThreads + threadIdx.x;
    if (e >= live) continue;
    const uint32_t kind = kr[j] & 15u, rank = kr[j] >> 4;
    q.perm[base + s_bin[(kind * kSortRounds + j) * kWaves + w] + rank] = base + e;
  }
}

// AOV (PRIMARY only): the first-hit position / id AOVs of RENDER_SPEC §13 are on — this sample's (P, hit) and ids go to ps.aov_pos /
// ps.aov_ids (each may be null).  A compile-time flag, like k_trace_primary's VIEWS: the variants without it compile exactly as before.
RT_DI void first_hit_aovs(const PathState& ps, uint32_t slot, float4 pos, uint4 ids) {
  if (ps.aov_pos) ps.aov_pos[slot] = pos;
  if (ps.aov_ids) ps.aov_ids[slot] = ids;
}
// GROUPS: the light groups of RENDER_SPEC §14 are on — every term added to the path's radiance also goes to its source's group sum
// (ps.groups), and light connections carry their light's group to the shadow pass.  A compile-time flag like AOV.
RT_DI void group_add(const PathState& ps, uint32_t g, uint32_t slot, f3 x) {
  P3* gp = ps.groups + (size_t)g * ps.group_stride + slot;
  const P3 l = *gp;
  *gp = P3{l.x + x.x, l.y + x.y, l.z + x.z};
}
template <bool PRIMARY, bool SIMPLE, bool SCATTER, bool AOV, bool GROUPS>
__global__ void __launch_bounds__(SIMPLE ? kShadeThreads : kShadeThreadsGeneric, SIMPLE ? RT_SHADE_WAVES_SIMPLE : RT_SHADE_WAVES) k_shade(FrameConst fc, SceneView sv, Queues q, PathState ps, Control* __restrict__ ctl, uint32_t depth) {
  __shared__ BlockCompact s_compact;
  const uint32_t n = PRIMARY ? fc.slot_count : ctl->sizes.n_active[depth];
  // the traversal of this bounce is over and the next users (shadow pass of this bounce, closest-hit pass of the next)
  // have not started: re-arm their work counters here
  if (blockIdx.x == 0u && threadIdx.x < kWorkShards) {
    ctl->work_closest.c[threadIdx.x * kWorkStride] = 0u;
    ctl->work_shadow[0].c[threadIdx.x * kWorkStride] = 0u;
    ctl->work_shadow[1].c[threadIdx.x * kWorkStride] = 0u;
    if (threadIdx.x == 0u) { ctl->work_closest.dry[0] = 0ull; ctl->work_shadow[0].dry[0] = 0ull; ctl->work_shadow[1].dry[0] = 0ull; }
  }
  uint32_t blk = blockIdx.x;
  if (!PRIMARY && !SIMPLE && sv.shade_sort) {
    // The workgroups that share a sort window read the same lines of the ray / state / hit queues (each takes a kind-slice of the
    // window's paths).  Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one, each XCD has its own L2): give every
    // window to ONE XCD — hardware blocks x, x + 8, x + 16, ... of a group of 8 windows take the consecutive logical blocks of window x.
    constexpr uint32_t kBPW = kSortWindow / kShadeThreadsGeneric, kGroup = 8u * kBPW;  // (the launcher rounds the grid up to whole groups)
    const uint32_t wi = blk % kGroup;
    blk = blk - wi + (wi & 7u) * kBPW + (wi >> 3);
  }
  if (blk * blockDim.x >= n) return;  // whole workgroup beyond the queue (uniform exit: barriers below)
  uint32_t i = blk * blockDim.x + threadIdx.x;
  // the texel decode table in LDS (shading.h::tex8_fetch); the barriers of the block compaction come long after every read of it
  __shared__ float s_tex_lut[SIMPLE ? 1 : kTexLutEntries];
  const RT_LDS float* lut = (const RT_LDS float*)s_tex_lut;
  if (!SIMPLE && sv.texture_count) {
    for (uint32_t k = threadIdx.x; k < kTexLutEntries; k += blockDim.x) s_tex_lut[k] = sv.tex_lut[k];
    __syncthreads();
  }
  if (!PRIMARY && !SIMPLE && sv.shade_sort && i < n) i = q.perm[i];  // kind order inside the window (k_shade_sort)
  const uint32_t in = depth & 1u, out = in ^ 1u;
  {
  const bool active = i < n;

  bool keep[3] = {false, false, false};  // path survives, light connection, environment connection
  f3 no = splat3(0.0f), nd = splat3(0.0f);
  float4 conn[2][3];  // the two NEE connections of this path, written to the compact queues after the block scan
  uint32_t slot = 0;
  f3 o, d;
  uint32_t rng = 0, rng_out = 0;                          // RNG counter on entry / for the next queue entry
  float4 state_out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // throughput | pdf for the next queue entry
  bool real = active;  // false: padding slot of a sharded frame (depth 0 only; later queues hold real paths only)
  if (PRIMARY && active) {
    slot = i;
    real = fc.views > 1u ? primary_ray<true>(fc, sv, slot, &o, &d, &rng) : primary_ray<false>(fc, sv, slot, &o, &d, &rng);  // wave-uniform
    if (fc.u.env_type == 1u) ps.radiance_env[slot] = P3{0.0f, 0.0f, 0.0f};
  }
  if (real) {
    // L: what this bounce adds to the path's radiance (at most one term: light hit | environment | emission)
    f3 T = splat3(1.0f), L = splat3(0.0f);
    uint32_t gL = 0;  // GROUPS: the light group of the source of L's term
    float prev_pdf = kNoNeePdf;  // no vertex has sampled a direction yet: an emitter reached through skipped (7.1d) surfaces counts in full
    if (!PRIMARY) {  // the whole state of a live path is its queue entry: coalesced reads, no gather by slot
      const float4* rp = reinterpret_cast<const float4*>(q.rays[in] + i);
      const float4 ro = rp[0], rd = rp[1], st = q.state[in][i];
      o = mk3(ro.x, ro.y, ro.z); d = mk3(rd.x, rd.y, rd.z);
      slot = __float_as_uint(ro.w); rng = __float_as_uint(rd.w);
      T = mk3(st.x, st.y, st.z); prev_pdf = st.w;
    }
    const float4 hv = reinterpret_cast<const float4*>(q.hits)[i];
    const uint32_t hit_word = __float_as_uint(hv.w);  // id << 3 | shading kind (hala_types.h: hit_encode) or kAbsent
    const uint32_t hit_prim = hit_word == kAbsent ? kAbsent : hit_word >> kHitKindBits;
    const uint32_t nl = fc.u.num_of_lights;
    const float t_surf = hit_prim != kAbsent ? hv.x : kTMax;

    int hit_light = -1;
    float t_light = t_surf, light_pdf = 0.0f;
    for (uint32_t k = 0; k < nl; ++k) {
      float lp;
      const float tl = intersect_light(sv.lights[k], o, d, &lp);
      if (tl > 0.0f && tl < t_light) { t_light = tl; hit_light = (int)k; light_pdf = lp; }
    }
    if (hit_light >= 0) {
      const f3 le = ld3(sv.lights[hit_light].intensity);
      float w = 1.0f;
      if (!PRIMARY) w = power_heuristic(prev_pdf, light_pdf * rcp_rn((float)nl));
      L = L + T * le * w;
      if (GROUPS) gL = ps.light_group[hit_light];
      if (PRIMARY) {
        ps.albedo[slot] = P3{minf(le.x, 1.0f), minf(le.y, 1.0f), minf(le.z, 1.0f)};
        ps.normal[slot] = P3{0.0f, 0.0f, 0.0f};
        if (AOV) {
          const f3 P = madd3(d, t_light, o);
          first_hit_aovs(ps, slot, make_float4(P.x, P.y, P.z, 1.0f), make_uint4(ps.light_node[hit_light], kAbsent, kAbsent, 0x80000000u | (uint32_t)hit_light));
        }
      }
    } else if (hit_prim == kAbsent) {
      f3 env;
      float w = 1.0f;
      if (fc.u.env_type == 1u) {
        env = env_map_eval(fc, sv, d);
        if (!PRIMARY) w = power_heuristic(prev_pdf, env_map_pdf(fc, sv, d));
      } else env = sky_eval(fc, d);
      L = L + T * env * w;
      if (GROUPS) gL = ps.env_group;
      if (PRIMARY) {
        ps.albedo[slot] = P3{minf(env.x, 1.0f), minf(env.y, 1.0f), minf(env.z, 1.0f)};
        ps.normal[slot] = P3{0.0f, 0.0f, 0.0f};
        if (AOV) first_hit_aovs(ps, slot, make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_uint4(kAbsent, kAbsent, kAbsent, kAbsent));
      }
    } else {
      // the LOD footprint of the path's own view at every depth (RENDER_SPEC §12); SIMPLE materials have no textures, one view keeps fc's
      float spread = fc.pixel_spread;
      if (!SIMPLE && fc.views > 1u) spread = view_pixel_spread(fc, slot);
      const Surface sf = make_surface<SIMPLE>(sv, lut, spread, o, d, hv.x, hv.y, hv.z, hit_prim);
      if (PRIMARY) {
        ps.albedo[slot] = P3{sf.mat.base.x, sf.mat.base.y, sf.mat.base.z};
        ps.normal[slot] = P3{sf.ns.x, sf.ns.y, sf.ns.z};
        if (AOV) first_hit_aovs(ps, slot, make_float4(sf.P.x, sf.P.y, sf.P.z, 1.0f), make_uint4(ps.inst_node[sf.inst], sf.inst, sf.material, hit_prim));
      }
      // the glow and the emission of this hit both come from the hit triangle's material: one group
      if (GROUPS) gL = ps.material_group[sf.material];
      // §7.1e: what the medium of an object just crossed did to the segment that ends here (identity for every other hit)
      if (sf.glow.x > 0.0f || sf.glow.y > 0.0f || sf.glow.z > 0.0f) {
        const f3 g = T * sf.glow;
        if (PRIMARY) L = L + g;
        else {  // a second term may follow in this bounce (emission): this one goes to the path's radiance right away, in order
          const P3 l = ps.radiance[slot];
          ps.radiance[slot] = P3{l.x + g.x, l.y + g.y, l.z + g.z};
          if (GROUPS) group_add(ps, gL, slot, g);
        }
      }
      T = T * sf.absorb;
      bool through = false, scattered = false;
      f3 pm = sf.P;        // the vertex the path is at: the surface point, or the scattering point inside the medium
      float hg_g = 0.0f;
      if (SCATTER && sf.sigma > 0.0f) {  // §7.1f: free flight through a scattering medium; the surface is only reached if the flight outlasts the segment
        const float rs = rng_next(rng);
        const float dist = -log_poly(1.0f - rs) / sf.sigma;
        if (dist < hv.x) {
          T = T * sf.scol;
          pm = madd3(d, dist, o);  // no offset: the point is inside the object
          hg_g = sf.hg;
          scattered = true;
        }
      }
      if (!scattered && sf.mat.opacity < 1.0f) {  // §7.1d: the surface is skipped with probability 1 - opacity (one extra random number)
        const float ro = rng_next(rng);
        through = !(ro < sf.mat.opacity);
      }
      if (through) {
        const bool alive = depth + 1u < fc.u.max_depth;
        keep[0] = alive;
        if (alive) {
          no = madd3(sf.ng, -sv.ray_eps, sf.P);
          nd = d;
        }
      } else {
      // a vertex with next-event estimation: a surface (BSDF, cosine, offset origin) or — §7.1f — a scattering point (Henyey-Greenstein
      // phase function: value = pdf, no cosine, the connection starts at the point itself and is attenuated on its way out by §7.1g)
      if (!scattered) {
        const f3 em = sf.mat.emission;
        if (em.x > 0.0f || em.y > 0.0f || em.z > 0.0f) L = L + T * em;
      }
      const f3 wo = -d;
      // the tangent frame, wo in it and the lobe weights of this vertex: shared by the two connections and the sampled continuation
      BsdfCtx bc{};
      if (!scattered) bc = bsdf_prepare(sf.mat, wo, sf.ns);
      if (nl > 0u) {  // NEE: one light
        const float rl = rng_next(rng), r1 = rng_next(rng), r2 = rng_next(rng);
        const uint32_t idx = min((uint32_t)(rl * (float)nl), nl - 1u);
        const LightSample ls = sample_light(sv.lights[idx], pm, r1, r2);
        if (ls.valid) {
          f3 fb; float pdf_b;
          if (scattered) { pdf_b = hg_phase(hg_g, dot3(d, ls.wi)); fb = splat3(pdf_b); }
          else bsdf_eval(sf.mat, bc, wo, ls.wi, sf.ns, &fb, &pdf_b);
          if (pdf_b > 0.0f) {
            const float side = dot3(ls.wi, sf.ng) >= 0.0f ? sv.ray_eps : -sv.ray_eps;
            const f3 so = scattered ? pm : madd3(sf.ng, side, sf.P);
            const float tmax = ls.dist >= kTMax ? kTMax : maxf(ls.dist - 2.0f * sv.ray_eps, 0.0f);
            const float cosl = scattered ? 1.0f : fabsf(dot3(sf.ns, ls.wi));  // |cos|: a connection may leave through the surface (§7.1c)
            f3 contrib;
            if (ls.delta) contrib = fb * ls.le * (cosl * (float)nl);
            else {
              const float pl = ls.pdf * rcp_rn((float)nl);
              const float w = power_heuristic(pl, pdf_b);
              contrib = fb * ls.le * (cosl * w / pl);
            }
            const f3 tc = T * contrib;
            conn[0][0] = make_float4(so.x, so.y, so.z, __uint_as_float(pcg_hash(rng ^ kAnyKeyLight)));  // tmin is 0: the field carries the any-hit key (7.1d)
            conn[0][1] = make_float4(ls.wi.x, ls.wi.y, ls.wi.z, tmax);
            conn[0][2] = make_float4(tc.x, tc.y, tc.z, __uint_as_float(GROUPS ? slot | (ps.light_group[idx] << kGroupShift) : slot));
            keep[1] = true;
          }
        }
      }
      if (fc.u.env_type == 1u) {  // NEE: environment map
        const float r1 = rng_next(rng), r2 = rng_next(rng);
        f3 wi; float pdf_e;
        if (env_map_sample(fc, sv, r1, r2, &wi, &pdf_e)) {
          f3 fb; float pdf_b;
          if (scattered) { pdf_b = hg_phase(hg_g, dot3(d, wi)); fb = splat3(pdf_b); }
          else bsdf_eval(sf.mat, bc, wo, wi, sf.ns, &fb, &pdf_b);
          if (pdf_b > 0.0f) {
            const float side = dot3(wi, sf.ng) >= 0.0f ? sv.ray_eps : -sv.ray_eps;
            const f3 so = scattered ? pm : madd3(sf.ng, side, sf.P);
            const float cosl = scattered ? 1.0f : fabsf(dot3(sf.ns, wi));
            const float w = power_heuristic(pdf_e, pdf_b);
            const f3 col = env_map_eval(fc, sv, wi);
            const f3 tc = T * (fb * col * (cosl * w / pdf_e));
            conn[1][0] = make_float4(so.x, so.y, so.z, __uint_as_float(pcg_hash(rng ^ kAnyKeyEnv)));
            conn[1][1] = make_float4(wi.x, wi.y, wi.z, kTMax);
            conn[1][2] = make_float4(tc.x, tc.y, tc.z, __uint_as_float(slot));
            keep[2] = true;
          }
        }
      }
      // continue the path
      f3 wi = d; bool sampled;
      if (scattered) {
        const float r1 = rng_next(rng), r2 = rng_next(rng);
        wi = hg_sample(d, hg_g, r1, r2);
        prev_pdf = hg_phase(hg_g, dot3(d, wi));  // the phase function is sampled exactly: throughput unchanged, the pdf goes to the next vertex's MIS weight
        sampled = true;
      } else {
        const float r1 = rng_next(rng), r2 = rng_next(rng), r3 = rng_next(rng);
        f3 fb; float pdf_b;
        sampled = bsdf_sample(sf.mat, bc, wo, sf.ns, r1, r2, r3, &wi, &fb, &pdf_b);
        if (sampled) { T = T * fb * (fabsf(dot3(sf.ns, wi)) / pdf_b); prev_pdf = pdf_b; }
      }
      if (sampled) {
        bool alive = true;
        if (depth >= fc.u.rr_depth) {
          const float qq = minf(max3f(T), 0.95f);
          const float rr = rng_next(rng);
          if (!(rr < qq)) alive = false; else T = T * rcp_rn(qq);
        }
        if (depth + 1u >= fc.u.max_depth) alive = false;
        keep[0] = alive;
        if (alive) {
          const float side = dot3(wi, sf.ng) >= 0.0f ? sv.ray_eps : -sv.ray_eps;
          no = scattered ? pm : madd3(sf.ng, side, sf.P);
          nd = wi;
        }
      }
      }  // !through
    }
    if (PRIMARY) {
      ps.radiance[slot] = P3{L.x, L.y, L.z};
      if (GROUPS)  // every group sum of the slot starts here: the term's group holds L, the others 0
        for (uint32_t g = 0; g < ps.group_count; ++g) ps.groups[(size_t)g * ps.group_stride + slot] = g == gL ? P3{L.x, L.y, L.z} : P3{0.0f, 0.0f, 0.0f};
    } else if (L.x != 0.0f || L.y != 0.0f || L.z != 0.0f) {  // radiance += term (this launch touches the word once: a plain update)
      const P3 l = ps.radiance[slot];
      ps.radiance[slot] = P3{l.x + L.x, l.y + L.y, l.z + L.z};
      if (GROUPS) group_add(ps, gL, slot, L);
    }
    rng_out = rng;
    state_out = make_float4(T.x, T.y, T.z, prev_pdf);
  }
  // ballot compaction (block level) of the surviving paths and of the two kinds of NEE connections
  uint32_t pos[3];
  uint32_t* const counters[3] = {&ctl->sizes.n_active[depth + 1u], &ctl->sizes.n_shadow[0][depth], &ctl->sizes.n_shadow[1][depth]};
  block_compact3(s_compact, keep, counters, &ctl->totals.rays_shadow, pos);
  if (keep[0]) {
    float4* rp = reinterpret_cast<float4*>(q.rays[out] + pos[0]);
    st4(rp, make_float4(no.x, no.y, no.z, __uint_as_float(slot)));
    st4(rp + 1, make_float4(nd.x, nd.y, nd.z, __uint_as_float(rng_out)));
    st4(&q.state[out][pos[0]], state_out);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (keep[1 + k]) {
      float4* ce = reinterpret_cast<float4*>(q.shadow[k] + pos[1 + k]);
      st4(ce, conn[k][0]); st4(ce + 1, conn[k][1]); st4(ce + 2, conn[k][2]);
    }
  }
  }
}
void launch_shade(const FrameConst& fc, const SceneView& sv, const Queues& q, const PathState& ps, Control* ctl, uint32_t depth, hipStream_t s) {
  const uint32_t threads = sv.simple_materials ? (uint32_t)kShadeThreads : (uint32_t)kShadeThreadsGeneric;
  dim3 grid(blocks_for(fc.slot_count, threads)), block(threads);
  // bounce launches of multi-kind scenes shade their paths in kind order inside windows of the queue
  if (depth != 0u && !sv.simple_materials && sv.shade_sort) {
    hipLaunchKernelGGL(k_shade_sort, dim3(blocks_for(fc.slot_count, kSortWindow)), dim3(kSortThreads), 0, s, q, ctl, depth);
    const uint32_t group = 8u * (kSortWindow / threads);  // whole groups of 8 windows: k_shade's window -> XCD mapping permutes the blocks of a group
    grid.x = blocks_for(grid.x, group) * group;
  }
  // the first-hit AOVs (RENDER_SPEC §13) are written by the depth-0 shade only; the light groups (§14) by every shade
  dispatch<kFamilyShade>([&](auto PRIMARY, auto SIMPLE, auto SCATTER, auto AOV, auto GROUPS) {
    hipLaunchKernelGGL((k_shade<PRIMARY, SIMPLE, SCATTER, AOV, GROUPS>), grid, block, 0, s, fc, sv, q, ps, ctl, depth);
  }, depth == 0u, sv.simple_materials != 0u, !sv.simple_materials && sv.scatter_media, depth == 0u && (ps.aov_pos || ps.aov_ids), ps.groups != nullptr);
}

}  // namespace rt
