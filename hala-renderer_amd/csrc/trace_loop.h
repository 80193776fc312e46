// trace_loop.h — the persistent wavefront loop of the traversal kernels (trace_closest.hip, trace_shadow.hip): the sharded dequeue,
// the loop around traverse.h's trav_step, the three ray sources (a ray batch, the camera, the NEE connections) and the kernels' prologue.
#pragma once
#include "shading.h"
#include "traverse.h"

namespace rt {
// Sharded dequeue of rays for the persistent kernels (see WorkCounters): the queue [0, n) is cut into kWorkShards
// contiguous shards, each with its own counter; a wave works on one shard until it is dry.  Wave-uniform.
struct WorkCursor {
  uint32_t shard, per;
  unsigned long long dead;  // shards that lie wholly beyond the queue's end: never probed
};
// Lane 0's value, to the whole wave.  Every caller runs with all 64 lanes of its wave active (the persistent loop is wave-uniform), so
// the first active lane IS lane 0 and the value comes back in a scalar register: what is decided from it (is the shard dry, is the
// queue dry) branches on the scalar unit instead of being carried as a lane mask through exec regions, as a ds_bpermute result was.
RT_DI uint32_t lane0_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
RT_DI unsigned long long lane0_u64(unsigned long long v) { return ((unsigned long long)lane0_u32((uint32_t)(v >> 32)) << 32) | lane0_u32((uint32_t)v); }
RT_DI bool lane_in(unsigned long long mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }  // this lane's bit of a wave-uniform mask, as a predicate: no instruction
RT_DI WorkCursor work_begin(uint32_t n) {
  WorkCursor c;
  const uint32_t batches = (n + kWorkBatch - 1u) / kWorkBatch;
  c.per = ((batches + kWorkShards - 1u) / kWorkShards) * kWorkBatch;  // rays per shard, a multiple of the batch
  const uint32_t live = c.per ? min(kWorkShards, (n + c.per - 1u) / c.per) : 0u;
  c.dead = live >= 64u ? 0ull : ~((1ull << live) - 1ull);
  c.shard = live ? blockIdx.x % live : 0u;
  return c;
}
// Variable-size dequeue for the refill loop: asks for `want` rays, is granted 1..want of them from one shard.
RT_DI uint32_t work_take(WorkCounters* wc, WorkCursor& c, uint32_t n, uint32_t want, uint32_t* got) {
  constexpr unsigned long long kAll = kWorkShards >= 64u ? ~0ull : (1ull << (kWorkShards & 63u)) - 1ull;
  if ((c.dead & kAll) == kAll) { *got = 0; return kAbsent; }
  for (;;) {
    uint32_t v = 0;
    if (lane_id() == 0u) v = atomicAdd(&wc->c[c.shard * kWorkStride], want);
    v = lane0_u32(v);
    const unsigned long long lo = (unsigned long long)c.shard * c.per + v;
    const unsigned long long hi = min((unsigned long long)(c.shard + 1u) * c.per, (unsigned long long)n);
    if (v < c.per && lo < hi) {
      *got = (uint32_t)min((unsigned long long)want, hi - lo);
      return (uint32_t)lo;
    }
    // this shard is dry: publish that (once) and move to a shard nobody has reported dry yet.  The mask only ever
    // gains bits and a bit is set only after the shard's last ray was handed out, so a stale read costs at most an
    // extra probe and "all dry" is never reported early.
    unsigned long long m = 0;
    if (lane_id() == 0u) {
      m = __hip_atomic_load(&wc->dry[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!(m & (1ull << c.shard))) { atomicOr(&wc->dry[0], 1ull << c.shard); m |= 1ull << c.shard; }
    }
    m = lane0_u64(m) | c.dead;
    if ((m & kAll) == kAll) { *got = 0; return kAbsent; }
    const unsigned long long avail = ~m & kAll;
    const uint32_t rot = (c.shard + 1u) & (kWorkShards - 1u);
    const unsigned long long r = rot ? (((avail >> rot) | (avail << (kWorkShards - rot))) & kAll) : avail;
    c.shard = (rot + (uint32_t)__ffsll((long long)r) - 1u) & (kWorkShards - 1u);
  }
}

// The persistent wavefront loop: every lane owns at most one ray in flight; whenever `refill` or more lanes are idle
// (and the queue is not dry) the wave dequeues exactly that many rays and hands them to its idle lanes by ballot rank
// — consecutive queue entries go to consecutive idle lanes, so refill loads stay as coalesced as the holes allow.
// Source: load(i, &o, &d, &tmin, &tmax) fetches queue entry i (false: no ray there); done(i, trav, payload) consumes the result.
template <bool ANY, bool COUNT, bool STAGED, bool ALPHA, bool INST, class Source>
RT_DI void persistent_trace(const SceneView& sv, const TraverseLds& lds, uint2* spill, WorkCounters* work, uint32_t n, uint32_t refill,
                            Source& src, StepCounters& sc) {
  WorkCursor cur = work_begin(n);
  bool more = n > 0u;  // wave-uniform: some shard may still hold rays
  // Which lanes hold a ray (`has`) and which hold a finished ray's result (`fin`) are 64-bit wave masks in scalar registers: the loop's
  // decisions (idle lanes, refill, end) are scalar arithmetic on them and scalar branches, and a lane's own bit is its predicate as it
  // stands (lane_in).  As per-lane bools they were merged through exec regions at every join and turned into masks and back through
  // the vector unit: ~25 scalar instructions per wave step.
  unsigned long long has = 0ull;
  uint32_t idx = 0;
  Trav t;
  typename Source::Payload pay;
  // Whole-wave batches (refill == 64: the LDS-staged scenes, whose rays are short) ask for their NEXT batch while the
  // current one is traced: the returning atomic's round trip (1-2 us, about as long as tracing 64 such rays) is off the
  // critical path.  A speculative request on a shard that has run dry just overshoots its counter; it is resolved —
  // taken if it lies inside the shard, else replaced by the searching dequeue — before anything else is asked for.
  bool pre_out = false;  // wave-uniform: a request is outstanding
  uint32_t pre_raw = 0, pre_shard = 0;
  // A finished ray keeps its result in the lane until the wave next refills (or ends): the results of all lanes that finished in
  // between leave in ONE store instruction — whole 1-KB runs for the whole-wave batches of the LDS-staged kernels (64 consecutive
  // queue entries: full lines for the nontemporal stores) — instead of one divergent store per lane and step.
  unsigned long long fin = 0ull;
  for (;;) {
    const unsigned long long idle = ~has;
    if (more && idle) {
      if (fin) {
        if (lane_in(fin)) src.done(idx, t, pay);
        fin = 0ull;
      }
      uint32_t got = 0, base = kAbsent;
      if (pre_out) {
        const uint32_t v = lane0_u32(pre_raw);
        const unsigned long long lo = (unsigned long long)pre_shard * cur.per + v;
        const unsigned long long hi = min((unsigned long long)(pre_shard + 1u) * cur.per, (unsigned long long)n);
        if (v < cur.per && lo < hi) { base = (uint32_t)lo; got = (uint32_t)min(64ull, hi - lo); }
        pre_out = false;
      }
      if (base == kAbsent) base = work_take(work, cur, n, (uint32_t)__popcll(idle), &got);
      if (base == kAbsent) more = false;
      else {
        if (STAGED && refill == 64u) {
          if (lane_id() == 0u) pre_raw = atomicAdd(&work->c[cur.shard * kWorkStride], 64u);
          pre_shard = cur.shard; pre_out = true;
        }
        bool took = false;
        if (lane_in(idle)) {
          const uint32_t rank = mbcnt64(idle);  // idle lanes below this one
          if (rank < got) {
            idx = base + rank;
            f3 o, d; float tmin, tmax; uint32_t key = 0u;
            if (src.load(idx, &o, &d, &tmin, &tmax, &key, &pay)) {  // false: the source had no ray for this entry and has dealt with it
              trav_begin(t, make_ray(o, d, tmin), tmax, key);
              took = true;
            }
          }
        }
        has |= __builtin_amdgcn_ballot_w64(took);
      }
    }
    if (has == 0ull) { if (!more) break; continue; }
    for (;;) {
      if (COUNT && lane_id() == 0u) sc.wave_steps++;  // lane 0 runs every iteration of this wave-uniform loop
      // every lane calls it: the large-scene variant deals the wave's leaf work out over all 64 lanes (traverse.h)
      trav_step<ANY, COUNT, STAGED, ALPHA, INST>(sv, lds, spill, t, lane_in(has), sc);
      const unsigned long long ended = __builtin_amdgcn_ballot_w64(t.cur == kAbsent) & has;  // a finished ray's mark (traverse.h); a lane without a ray holds anything
      fin |= ended; has &= ~ended;
      const uint32_t nidle = 64u - (uint32_t)__popcll(has);
      if (nidle == 64u || (more && nidle >= refill)) break;
    }
  }
  if (lane_in(fin)) src.done(idx, t, pay);
}

struct BatchSource {
  struct Payload {};
  const hala_ray* rays;
  hala_hit* hits;
  bool any;
  bool queue;  // the renderer's own bounce-ray queue: tmin = 0, tmax = FLT_MAX, their fields carry path slot and RNG counter
  // Hit records of whole-wave batches (LDS-staged kernels) leave as full 1-KB runs: nontemporal stores.  Per-lane refills finish
  // scattered entries at scattered times: ordinary stores, so that L2 puts the 16-B pieces of a line together before it goes to
  // memory (nontemporal 16-B pieces reached the fabric at 1.8-2.1x their bytes: profiles/r01_m_pmc_config2.txt, r02_a_pmc_config4).
  bool streaming;
  RT_DI bool load(uint32_t i, f3* o, f3* d, float* tmin, float* tmax, uint32_t* key, Payload*) const {
    const float4* rp = reinterpret_cast<const float4*>(rays + i);
    const float4 ro = rp[0], rd = rp[1];
    *o = mk3(ro.x, ro.y, ro.z); *d = mk3(rd.x, rd.y, rd.z); *tmin = queue ? 0.0f : ro.w; *tmax = queue ? kTMax : rd.w;
    if (any) *key = pcg_hash(i ^ kAnyKeyBatch);  // RENDER_SPEC 7.1d: the key of ray i of a batch
    return true;
  }
  RT_DI void done(uint32_t i, const Trav& t, const Payload&) const {
    const bool found = t.best.prim != kAbsent;
    float4 out;
    if (any) out = make_float4(found ? 1.0f : -1.0f, 0.0f, 0.0f, __uint_as_float(kAbsent));
    // the renderer's own queue keeps id << 3 | shading kind (hala_types.h: hit_encode); a caller's batch gets the plain triangle id
    else out = found ? make_float4(t.best.t, t.best.u, t.best.v, __uint_as_float(queue ? t.best.prim : t.best.prim >> kHitKindBits)) : make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(kAbsent));
    if (streaming) st4(reinterpret_cast<float4*>(hits) + i, out);
    else reinterpret_cast<float4*>(hits)[i] = out;
  }
};
// FAR: a camera ray may start beyond the scene's far limit (RENDER_SPEC 4.2; the host decides from the camera records): every ray is
// tested and, if far, re-based as it is set up; the distance it was moved travels with the lane and comes back on the hit's t.  A
// separate variant: the kernels of every other frame stay as they are, to the register.
template <bool FAR> struct CameraPayload {};
template <> struct CameraPayload<true> { float ts; };
template <bool VIEWS, bool FAR>
struct CameraSource {
  typedef CameraPayload<FAR> Payload;
  const FrameConst& fc;
  const SceneView& sv;
  hala_hit* hits;
  bool streaming;
  RT_DI bool load(uint32_t i, f3* o, f3* d, float* tmin, float* tmax, uint32_t*, Payload* p) const {
    uint32_t rng;
    *tmin = 0.0f; *tmax = kTMax;
    if (primary_ray<VIEWS>(fc, sv, i, o, d, &rng)) {
      if constexpr (FAR) p->ts = rebase_ray(sv, *o, *d, *tmin, *tmax);
      return true;
    }
    reinterpret_cast<float4*>(hits)[i] = make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(kAbsent));  // padding slot: no ray
    return false;
  }
  RT_DI void done(uint32_t i, const Trav& t, const Payload& p) const {
    const bool found = t.best.prim != kAbsent;
    float bt = t.best.t;
    if constexpr (FAR) bt += p.ts;
    const float4 out = found ? make_float4(bt, t.best.u, t.best.v, __uint_as_float(t.best.prim)) : make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(kAbsent));
    if (streaming) st4(reinterpret_cast<float4*>(hits) + i, out);
    else reinterpret_cast<float4*>(hits)[i] = out;
  }
};
template <bool ALPHA, bool GROUPS>
struct ShadowSource {
  // contribution.xyz | pixel slot, fetched with the ray (one coalesced 48-B record), and the path's radiance as it stands
  struct Payload { float4 cs; float lx, ly, lz; };
  const ShadowEntry* entries;
  P3* radiance;
  // GROUPS (RENDER_SPEC §14): the light connections' entries carry slot | group << kGroupShift, and an unoccluded one adds its contribution
  // to that group's sum of the path too — the same owner rule, one IEEE add per component.  Null for the environment connections.
  P3* groups;
  uint32_t group_stride;
  // A path owns at most one connection per queue and the two queues add to different arrays, so nothing else touches this word of the
  // path's radiance during the launch: it is fetched here, behind the entry (the load is in flight while the ray is traced), and
  // an unoccluded ray stores radiance + contribution — one IEEE add per component, no ordering freedom.  (Three memory-side float
  // atomics per unoccluded ray did the same and cost 57 of the launch's 160 us on the headline config: profiles/r01_h_experiments.txt.)
  // The two connection kinds of a bounce share a launch but not an array: light connections add to L, environment connections to Le.
  RT_DI bool load(uint32_t i, f3* o, f3* d, float* tmin, float* tmax, uint32_t* key, Payload* p) const {
    const float4* e = reinterpret_cast<const float4*>(entries + i);
    const float4 ro = e[0], rd = e[1];
    p->cs = e[2];
    const uint32_t slot = GROUPS ? (__float_as_uint(p->cs.w) & kGroupSlotMask) : __float_as_uint(p->cs.w);
    const float* l = reinterpret_cast<const float*>(radiance + slot);
    p->lx = l[0]; p->ly = l[1]; p->lz = l[2];
    // a connection starts at its origin (tmin = 0): the field carries its any-hit key (RENDER_SPEC 7.1d)
    *o = mk3(ro.x, ro.y, ro.z); *d = mk3(rd.x, rd.y, rd.z); *tmin = 0.0f; *tmax = rd.w; *key = __float_as_uint(ro.w);
    return true;
  }
  RT_DI void done(uint32_t, const Trav& t, const Payload& p) const {
    if (t.best.prim != kAbsent) return;  // occluded
    float cx = p.cs.x, cy = p.cs.y, cz = p.cs.z;
    if (ALPHA && (t.tau[0] | t.tau[1] | t.tau[2])) {  // RENDER_SPEC 7.1g: what the media the connection crossed leave of it
      const f3 tr = any_transmittance(t.tau);
      if (tr.x != 1.0f || tr.y != 1.0f || tr.z != 1.0f) { cx = cx * tr.x; cy = cy * tr.y; cz = cz * tr.z; }
    }
    const uint32_t w = __float_as_uint(p.cs.w), slot = GROUPS ? (w & kGroupSlotMask) : w;
    float* l = reinterpret_cast<float*>(radiance + slot);
    l[0] = p.lx + cx; l[1] = p.ly + cy; l[2] = p.lz + cz;
    if (GROUPS && groups) {
      P3* gp = groups + (size_t)(w >> kGroupShift) * group_stride + slot;
      const P3 g = *gp;
      *gp = P3{g.x + cx, g.y + cy, g.z + cz};
    }
  }
};
// the connections of kind 0 (light: they add to L and carry a group) or 1 (environment: they add to Le) of one bounce
template <bool ALPHA, bool GROUPS>
RT_DI ShadowSource<ALPHA, GROUPS> shadow_source(const Queues& q, const PathState& ps, uint32_t kind) {
  return ShadowSource<ALPHA, GROUPS>{q.shadow[kind], kind ? ps.radiance_env : ps.radiance, kind ? nullptr : ps.groups, ps.group_stride};
}

// What every trace kernel starts with: its LDS (stage_bvh on g_smem), this lane's slice of the global stack spill area (null: the
// scene's stacks fit the LDS entries) and the lane's tallies (StepCounters).
extern __shared__ __attribute__((aligned(16))) unsigned char g_smem[];
RT_DI uint2* lane_spill(uint2* spill_base) { return spill_base ? spill_base + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * kStackSpill : nullptr; }

// counting launches: one set of atomics per wave
RT_DI void flush_counters(Control* ctl, int kind, const StepCounters& sc) {
  const uint32_t v[5] = {wave_sum(sc.nodes), wave_sum(sc.tris), wave_sum(sc.wave_steps), wave_sum(sc.leaf_passes), wave_sum(sc.leaf_lanes)};
  if (lane_id() != 0u) return;
  atomicAdd(&ctl->totals.steps[kind][0], (unsigned long long)v[0]); atomicAdd(&ctl->totals.steps[kind][1], (unsigned long long)v[1]);
  atomicAdd(&ctl->totals.probe[kind][0], (unsigned long long)v[2]); atomicAdd(&ctl->totals.probe[kind][1], (unsigned long long)v[3]);
  atomicAdd(&ctl->totals.probe[kind][2], (unsigned long long)v[4]);
}

}  // namespace rt
