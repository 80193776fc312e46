// rt_tiles.hip — the frame distributed over ranks: the tile shard (RENDER_SPEC 9), the scatter of gathered tiles and the RCCL
// exchange (ExchangeState).
#include "renderer_state.h"

namespace rt {

static uint32_t gcd_u32(uint32_t a, uint32_t b) { while (b) { uint32_t t = a % b; a = b; b = t; } return a; }
static uint32_t mod_inverse(uint32_t a, uint32_t n) {  // a^-1 mod n (a, n coprime); n == 1 -> 0
  long long t = 0, nt = 1, r = n, nr = a % n;
  while (nr != 0) { long long q = r / nr; long long tmp = t - q * nt; t = nt; nt = tmp; tmp = r - q * nr; r = nr; nr = tmp; }
  if (t < 0) t += n;
  return (uint32_t)t;
}

void compute_tiling(hala_rt_renderer* r) {
  if (r->world <= 1) {
    r->real_pixels = r->width * r->height;
    r->slot_count = r->real_pixels;
    r->blocks_x = 0;
    if (kPixelBlock) {  // whole blocks: the border blocks of a frame that is not a multiple of the block size hold padding slots
      r->blocks_x = (r->width + kPixelBlock - 1) / kPixelBlock;
      r->slot_count = r->blocks_x * ((r->height + kPixelBlock - 1) / kPixelBlock) * kPixelBlock * kPixelBlock;
    }
    r->tiles_x = r->tiles_y = r->tiles_per_rank = 0;
    return;
  }
  r->tiles_x = (r->width + r->tile_size - 1) / r->tile_size;
  r->tiles_y = (r->height + r->tile_size - 1) / r->tile_size;
  const uint32_t n = r->tiles_x * r->tiles_y;
  r->tiles_per_rank = (n + r->world - 1) / r->world;
  uint32_t A = 0x9E3779B1u % n;  // RENDER_SPEC §9: perm(t) = (t*A + B) mod n, A coprime to n
  if (A == 0) A = 1;
  while (gcd_u32(A, n) != 1) ++A;
  r->perm_a_inv = mod_inverse(A, n);
  r->perm_b = 7;
  r->slot_count = r->tiles_per_rank * r->tile_size * r->tile_size;
  // pixels this rank really owns (its padding tiles and the out-of-frame part of border tiles hold no paths)
  uint64_t real = 0;
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t k = (uint32_t)(((uint64_t)t * A + r->perm_b) % n);
    if (k % r->world != r->rank) continue;
    const uint32_t tx = t % r->tiles_x, ty = t / r->tiles_x;
    const uint32_t w = std::min(r->tile_size, r->width - tx * r->tile_size), h = std::min(r->tile_size, r->height - ty * r->tile_size);
    real += (uint64_t)w * h;
  }
  r->real_pixels = (uint32_t)real;
}

}  // namespace rt

extern "C" {

// ---- multi-GPU tiles ------------------------------------------------------------------------------------------------
int hala_rt_set_tile_shard(hala_rt_renderer* r, uint32_t rank, uint32_t world, uint32_t tile_size) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (world == 0 || rank >= world) RT_FAIL("Invalid rank / world size.");
  if (tile_size == 0 || tile_size > 256) RT_FAIL("Invalid tile size.");
  if (world > 1 && r->adaptive.enabled) RT_FAIL("Adaptive sampling is on: a sharded frame cannot use it (hala_rt_set_adaptive_sampling(r, NULL) first).");
  if (world > 1 && r->view_count() > 1u) RT_FAIL("The renderer has several views: a sharded frame renders one (hala_rt_set_views with one camera first).");
  if (world > 1 && r->groups.count) RT_FAIL("Light groups are on: a sharded frame cannot use them (hala_rt_set_light_groups(r, NULL) first).");
  if (world > 1 && r->crypto.mask) RT_FAIL("Cryptomatte is on: a sharded frame cannot use it (hala_rt_set_cryptomatte(r, NULL) first).");
  if (world > 1 && r->temporal.enabled) RT_FAIL("Temporal reprojection is on: a sharded frame cannot use it (hala_rt_set_temporal(r, NULL) first).");
  // a collective in flight belongs to the old shard: complete it (its receive buffer is laid out for the old world size)
  if (r->exchange.pending && hala_rt_tile_allgather_finish(r) != HALA_OK) return HALA_ERR;
  // a communicator is bound to (rank, world): gather_recv is sized by it and the de-interleave indexes it by the shard's world
  if (r->exchange.comm && ((uint32_t)r->exchange.comm_rank != rank || (uint32_t)r->exchange.comm_world != world))
    RT_FAIL("The renderer holds a communicator for rank " + std::to_string(r->exchange.comm_rank) + " of " + std::to_string(r->exchange.comm_world) +
            ": call hala_rt_comm_destroy before changing the tile shard.");
  RT_HIP(hipStreamSynchronize(r->stream));
  if (r->exchange.stream) RT_HIP(hipStreamSynchronize(r->exchange.stream));
  r->rank = rank; r->world = world; r->tile_size = tile_size;
  r->temporal.drop_history();  // RENDER_SPEC §16
  compute_tiling(r);
  if (alloc_frame_buffers(r) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  r->reset_accumulation();
  return HALA_OK;
}
int hala_rt_tile_buffer(hala_rt_renderer* r, int which, void** d_ptr, size_t* bytes) {
  if (!r || !r->has_image(which) || !d_ptr || !bytes) RT_FAIL("Invalid argument.");
  *d_ptr = r->img_local[which].ptr;
  *bytes = r->image_pixels() * sizeof(float4);
  return HALA_OK;
}
int hala_rt_get_stream(hala_rt_renderer* r, void** hip_stream) {
  if (!hip_stream) RT_FAIL("Invalid argument.");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  *hip_stream = static_cast<void*>(r->stream);
  return HALA_OK;
}
int hala_rt_scatter_gathered_tiles_on_stream(hala_rt_renderer* r, int which, const void* d_gathered, size_t bytes, void* hip_stream) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->has_image(which) || !d_gathered) RT_FAIL("Invalid argument.");
  if (r->world <= 1) RT_FAIL("The renderer is not sharded.");
  if (bytes != r->image_pixels() * r->world * sizeof(float4)) RT_FAIL("The gathered buffer has the wrong size.");
  RT_HIP(r->img_full[which].resize((size_t)r->width * r->height));
  hala_global_uniform u = r->last_uniform;
  const FrameConst fc = r->frame_const(u);
  launch_scatter_tiles(fc, static_cast<const float4*>(d_gathered), r->img_full[which].ptr, hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream);  // stream ordered: readers wait themselves
  RT_HIP(hipGetLastError());
  r->full_valid[which] = true;
  return HALA_OK;
}
int hala_rt_scatter_gathered_tiles(hala_rt_renderer* r, int which, const void* d_gathered, size_t bytes) {
  return hala_rt_scatter_gathered_tiles_on_stream(r, which, d_gathered, bytes, nullptr);
}


// ---- RCCL tile all-gather (BASELINE.json north_star: "RCCL all-gather of tiles over xGMI") -----------------------------------------
// librccl is resolved on first use (dyn_api.h): a one-GPU host loads libhalart.so without it.
#define RT_RCCL_API(api)                                   \
  std::string _rccl_err;                                   \
  const RcclApi* api = rccl_api(&_rccl_err);               \
  if (!api) RT_FAIL(_rccl_err)
#define RT_NCCL(api, expr)                                                                                         \
  do {                                                                                                             \
    const ncclResult_t _r = (expr);                                                                                \
    if (_r != ncclSuccess) RT_FAIL(std::string("RCCL: ") + (api)->GetErrorString(_r) + " (" #expr ")");            \
  } while (0)

int hala_rt_comm_unique_id(void* out_128_bytes) {
  if (!out_128_bytes) RT_FAIL("Invalid argument.");
  static_assert(sizeof(ncclUniqueId) == HALA_COMM_UNIQUE_ID_BYTES, "ncclUniqueId is 128 bytes");
  RT_RCCL_API(api);
  ncclUniqueId id;
  RT_NCCL(api, api->GetUniqueId(&id));
  memcpy(out_128_bytes, &id, sizeof(id));
  return HALA_OK;
}
// the side stream and the three hand-over events of the exchange (with or without a communicator)
static int ensure_gather_resources(hala_rt_renderer* r) {
  if (!r->exchange.stream) RT_HIP(hipStreamCreateWithFlags(&r->exchange.stream, hipStreamNonBlocking));
  for (hipEvent_t* e : {&r->exchange.ev_rendered, &r->exchange.ev_staged, &r->exchange.ev_gathered}) if (!*e) RT_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  return HALA_OK;
}
static int comm_common(hala_rt_renderer* r, int rank, int world) {
  if ((uint32_t)world != r->world || (uint32_t)rank != r->rank)
    RT_FAIL("The communicator's rank / size (" + std::to_string(rank) + " / " + std::to_string(world) + ") differ from the renderer's tile shard (" +
            std::to_string(r->rank) + " / " + std::to_string(r->world) + "): call hala_rt_set_tile_shard first.");
  r->exchange.comm_rank = rank; r->exchange.comm_world = world;
  return ensure_gather_resources(r);
}
int hala_rt_comm_init_rank(hala_rt_renderer* r, const void* unique_id_128_bytes, uint32_t rank, uint32_t world) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!unique_id_128_bytes || world == 0 || rank >= world) RT_FAIL("Invalid argument.");
  if (r->exchange.comm) RT_FAIL("The renderer already has a communicator.");
  RT_RCCL_API(api);
  if (comm_common(r, (int)rank, (int)world) != HALA_OK) return HALA_ERR;
  ncclUniqueId id;
  memcpy(&id, unique_id_128_bytes, sizeof(id));
  RT_NCCL(api, api->CommInitRank(&r->exchange.comm, (int)world, id, (int)rank));
  r->exchange.comm_owned = true;
  return HALA_OK;
}
int hala_rt_comm_attach(hala_rt_renderer* r, void* nccl_comm) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!nccl_comm) RT_FAIL("Invalid argument.");
  if (r->exchange.comm) RT_FAIL("The renderer already has a communicator.");
  RT_RCCL_API(api);
  int rank = 0, world = 0;
  RT_NCCL(api, api->CommUserRank(static_cast<ncclComm_t>(nccl_comm), &rank));
  RT_NCCL(api, api->CommCount(static_cast<ncclComm_t>(nccl_comm), &world));
  if (comm_common(r, rank, world) != HALA_OK) return HALA_ERR;
  r->exchange.comm = static_cast<ncclComm_t>(nccl_comm);
  r->exchange.comm_owned = false;
  return HALA_OK;
}
int hala_rt_comm_destroy(hala_rt_renderer* r) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (r->exchange.stream) RT_HIP(hipStreamSynchronize(r->exchange.stream));
  if (r->exchange.comm && r->exchange.comm_owned) {
    RT_RCCL_API(api);
    RT_NCCL(api, api->CommDestroy(r->exchange.comm));
  }
  r->exchange.comm = nullptr; r->exchange.comm_owned = false; r->exchange.pending = 0;
  return HALA_OK;
}

// finish(k - 1) -> [side stream waits for the renderer's stream: frame k is complete] -> staging <- tiles -> [renderer's stream waits
// for that copy: frame k + 1 may overwrite the tiles] -> the exchange (receive <- every rank's staging) on the side stream.  Nothing
// blocks the host.  external = false: the exchange is ncclAllGather on the renderer's communicator.  external = true
// (hala_rt_tile_allgather_begin_external): the CALLER performs it — a host with another transport (MPI, a gloo rehearsal on one GPU,
// tests that emulate the ranks) reads the staging buffer and fills the receive buffer on the exchange stream (hala_rt_get_exchange_buffers) —
// everything else (staging copy, event order, de-interleave in finish) is this very code.
static int allgather_begin(hala_rt_renderer* r, uint32_t aov_mask, bool external) {
  // bits 4 and 5: the first-hit AOVs, while on (RENDER_SPEC §13)
  if (aov_mask == 0u || aov_mask > 63u || ((aov_mask >> 4) & ~r->aov_mask)) RT_FAIL("Invalid AOV mask.");
  if (hala_rt_tile_allgather_finish(r) != HALA_OK) return HALA_ERR;
  if (ensure_gather_resources(r) != HALA_OK) return HALA_ERR;
  const uint32_t world = external ? r->world : (uint32_t)r->exchange.comm_world;
  if (world != r->world) RT_FAIL("The communicator's size differs from the renderer's tile shard.");  // (set_tile_shard refuses the change)
  const size_t n = r->image_pixels();
  hipStream_t g = r->exchange.stream;
  RT_HIP(hipEventRecord(r->exchange.ev_rendered, r->stream));
  RT_HIP(hipStreamWaitEvent(g, r->exchange.ev_rendered, 0));
  for (int which = 0; which < 6; ++which) {
    if (!(aov_mask & (1u << which))) continue;
    RT_HIP(r->exchange.stage[which].resize(n));
    RT_HIP(r->exchange.recv[which].resize(n * (size_t)world));
    RT_HIP(hipMemcpyAsync(r->exchange.stage[which].ptr, r->img_local[which].ptr, n * sizeof(float4), hipMemcpyDeviceToDevice, g));
  }
  RT_HIP(hipEventRecord(r->exchange.ev_staged, g));
  RT_HIP(hipStreamWaitEvent(r->stream, r->exchange.ev_staged, 0));
  if (!external) {
    RT_RCCL_API(api);
    for (int which = 0; which < 6; ++which)
      if (aov_mask & (1u << which))
        RT_NCCL(api, api->AllGather(r->exchange.stage[which].ptr, r->exchange.recv[which].ptr, n * 4, ncclFloat, r->exchange.comm, g));
  }
  r->exchange.pending = aov_mask;
  return HALA_OK;
}
int hala_rt_tile_allgather_begin(hala_rt_renderer* r, uint32_t aov_mask) {
  RtRange range("halart::tile_allgather_begin");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->exchange.comm) RT_FAIL("The renderer has no communicator: call hala_rt_comm_init_rank or hala_rt_comm_attach first.");
  return allgather_begin(r, aov_mask, false);
}
int hala_rt_tile_allgather_begin_external(hala_rt_renderer* r, uint32_t aov_mask) {
  RtRange range("halart::tile_allgather_begin_external");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  return allgather_begin(r, aov_mask, true);
}
int hala_rt_get_exchange_buffers(hala_rt_renderer* r, int which, void** d_staged, size_t* staged_bytes, void** d_receive, size_t* receive_bytes, void** hip_stream) {
  if (!r || !r->has_image(which)) RT_FAIL("Invalid argument.");
  if (!(r->exchange.pending & (1u << which))) RT_FAIL("No exchange of this image is in flight: call hala_rt_tile_allgather_begin_external first.");
  if (d_staged) *d_staged = r->exchange.stage[which].ptr;
  if (staged_bytes) *staged_bytes = r->exchange.stage[which].bytes();
  if (d_receive) *d_receive = r->exchange.recv[which].ptr;
  if (receive_bytes) *receive_bytes = r->exchange.recv[which].bytes();
  if (hip_stream) *hip_stream = static_cast<void*>(r->exchange.stream);
  return HALA_OK;
}
// de-interleave on the side stream (beside the rendering of the next frame), then whatever the renderer's stream does next — and
// whoever waits for it — sees the row-major images complete
int hala_rt_tile_allgather_finish(hala_rt_renderer* r) {
  RtRange range("halart::tile_allgather_finish");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->exchange.pending) return HALA_OK;
  const uint32_t mask = r->exchange.pending;
  r->exchange.pending = 0;
  hipStream_t g = r->exchange.stream;
  if (r->world > 1) {
    const FrameConst fc = r->frame_const(r->last_uniform);
    for (int which = 0; which < 6; ++which) {
      if (!(mask & (1u << which))) continue;
      if (r->exchange.recv[which].count != r->image_pixels() * (size_t)r->world) RT_FAIL("The receive buffer does not match the tile shard.");
      RT_HIP(r->img_full[which].resize((size_t)r->width * r->height));
      launch_scatter_tiles(fc, r->exchange.recv[which].ptr, r->img_full[which].ptr, g);
      r->full_valid[which] = true;
    }
  }
  RT_HIP(hipEventRecord(r->exchange.ev_gathered, g));
  RT_HIP(hipStreamWaitEvent(r->stream, r->exchange.ev_gathered, 0));
  RT_HIP(hipGetLastError());
  return HALA_OK;
}
int hala_rt_tile_allgather(hala_rt_renderer* r, uint32_t aov_mask) {
  if (hala_rt_tile_allgather_begin(r, aov_mask) != HALA_OK) return HALA_ERR;
  return hala_rt_tile_allgather_finish(r);
}
int hala_rt_get_gathered_buffer(hala_rt_renderer* r, int which, void** d_ptr, size_t* bytes) {
  if (!r || !r->has_image(which) || !d_ptr || !bytes) RT_FAIL("Invalid argument.");
  *d_ptr = r->exchange.recv[which].ptr;
  *bytes = r->exchange.recv[which].bytes();
  return HALA_OK;
}

}  // extern "C"
