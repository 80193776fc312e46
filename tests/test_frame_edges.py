"""Frame geometry at its edges (docs/RENDER_SPEC.md §9): the path slot -> pixel maps (slot_to_pixel, compute_tiling, k_scatter_tiles)
at resolutions and tile shards the other GPU tests never reach.  Unsharded frames smaller than one 8 x 8 pixel block, one pixel wide or
high, or not a multiple of 8, against the CPU oracle; sharded layouts with in-tile row-major order, tiles of 1 and 256, a tile larger
than the frame and more ranks than tiles, against the unsharded frame (itself held to the oracle); and the shards
hala_rt_set_tile_shard refuses.  Every image comparison is bit for bit."""
import numpy as np
import pytest

from hala_renderer_amd import scenes
from hala_renderer_amd.dist import TileLayout

pytestmark = pytest.mark.gpu

EDGE_SIZES = [(1, 1), (1, 29), (29, 1), (5, 3), (8, 8), (9, 9), (7, 64), (64, 7), (61, 37)]
# (w, h, tile_size, world): in-tile row-major order (ts % 8 != 0) with partial border tiles; a multiple of 8 that is not a power of two;
# ts = 1; one tile larger than the frame (ranks 1 and 2 own nothing); more ranks than tiles; ts = 8 with one 8 x 8 block per tile
SHARD_LAYOUTS = [(61, 37, 7, 3), (61, 37, 12, 5), (200, 120, 40, 3), (23, 17, 1, 4), (100, 70, 256, 3), (40, 24, 16, 8), (1, 1, 32, 2),
                 (33, 17, 8, 8)]
SPP = 2


def layout_id(p):
    w, h, ts, world = p
    return f"{w}x{h}-ts{ts}-world{world}"


def assert_same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.any(got != want, axis=-1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ")


def edge_scene(kind, w, h):
    """(scene, envmap, max_depth, rr_depth, tonemap).  "cornell": one material kind (the SIMPLE shade kernels), a tree small enough to
    be staged in LDS.  "blob": Disney and Lambert materials under an env map (the generic shade kernels and k_shade_sort), tonemapped."""
    if kind == "cornell":
        return scenes.cornell_box(aspect=w / h), None, 5, 3, (False, False, False)
    return (scenes.bunny_class(subdivisions=4, aspect=w / h, disney=True), scenes.sky_sun_envmap(128, 64, sun_gain=300.0), 4, 2,
            (True, True, False))


def renderer(halart, kind, w, h, shard=None):
    scene, env, md, rr, tm = edge_scene(kind, w, h)
    r = halart.HalaRenderer("edges", w, h, md, rr, *tm, 0)
    if shard is not None:
        r.set_tile_shard(*shard)
    if env is not None:
        r.set_envmap(env, 40.0)
    r.set_scene(scene)
    r.commit()
    return r


def oracle_render(oracle, kind, w, h, frames):
    scene, env, md, rr, tm = edge_scene(kind, w, h)
    return oracle.OracleScene(scene, envmap=env).render(w, h, frames=frames, max_depth=md, rr_depth=rr, tonemap=tm,
                                                        env_rotation=40.0 if env is not None else 0.0)


@pytest.mark.parametrize("kind", ["cornell", "blob"])
@pytest.mark.parametrize("w,h", EDGE_SIZES)
def test_unsharded_edge_resolution_against_the_oracle(halart, oracle, kind, w, h):
    """update() twice, then a new accumulation through update_batch(3) (path slot k * pixel_slots + pslot): all four images equal
    the oracle's, and the ray totals are the oracle's with w * h camera rays per sample"""
    r = renderer(halart, kind, w, h)
    try:
        assert (r.bvh_info().lds_node_count > 0) == (kind == "cornell")  # the LDS-staged traversal variants, or the large-scene ones
        r.update(); r.update(); r.render()
        want, ost = oracle_render(oracle, kind, w, h, 2)
        for k, name in enumerate(("accum", "albedo", "normal", "final")):
            assert_same(r.read_image(k), want[k], f"update x2 {name}")
        st = r.statistics()
        assert st.rays_primary_total == w * h * 2
        assert (st.rays_closest_total, st.rays_shadow_total) == (ost.rays_closest, ost.rays_shadow)
        r.reset_accumulation()
        r.update_batch(3)
        want, ost3 = oracle_render(oracle, kind, w, h, 3)
        for k, name in enumerate(("accum", "albedo", "normal", "final")):
            assert_same(r.read_image(k), want[k], f"update_batch(3) {name}")
        st = r.statistics()
        assert st.rays_primary_total == w * h * 5
        assert (st.rays_closest_total, st.rays_shadow_total) == (ost.rays_closest + ost3.rays_closest, ost.rays_shadow + ost3.rays_shadow)
    finally:
        r.close()


def tile_buffers(halart, r, L):
    """the rank's four tile buffers (accum, albedo, normal, final), copied off the device"""
    import torch
    r.wait_idle()
    out = []
    for k in range(4):
        ptr, nbytes = r.tile_buffer(k)
        assert nbytes == L.pixels_per_rank * 16
        out.append(torch.as_tensor(halart.dist._DeviceView(ptr, nbytes // 4), device="cuda:0").clone())
    torch.cuda.synchronize()  # the copies run on torch's stream: done before the renderer's stream writes the tile buffers again
    return out


@pytest.mark.parametrize("layout", SHARD_LAYOUTS, ids=layout_id)
def test_sharded_layout_equals_the_unsharded_frame(halart, oracle, layout):
    """the ranks are emulated one after another on one GPU.  The unsharded frame is held to the oracle; every rank's tile buffers, in
    all_gather_into_tensor order, must give that frame back through TileLayout.unshard and through the library's k_scatter_tiles, for
    SPP update()s and for update_batch(SPP), and hold zeros in their padding slots; summed over the ranks the ray totals are the
    unsharded frame's"""
    import torch
    w, h, ts, world = layout
    L = TileLayout(w, h, world, ts)
    ref = renderer(halart, "cornell", w, h)
    try:
        for _ in range(SPP):
            ref.update()
        ref.render()
        want = [ref.read_image(k) for k in range(3)]
        oimg, ost = oracle_render(oracle, "cornell", w, h, SPP)
        for k in range(3):
            assert_same(want[k], oimg[k], f"unsharded AOV {k} against the oracle")
        ref.reset_accumulation()
        ref.update_batch(SPP)
        for k in range(3):
            assert_same(ref.read_image(k), want[k], f"unsharded update_batch AOV {k}")
        rst = ref.statistics()
        assert (rst.rays_closest_total, rst.rays_shadow_total) == (2 * ost.rays_closest, 2 * ost.rays_shadow)
    finally:
        ref.close()

    shards = {"update": [[] for _ in range(3)], "batch": [[] for _ in range(3)]}
    primary = closest = shadow = 0
    last = None
    try:
        for rank in range(world):
            r = renderer(halart, "cornell", w, h, shard=(rank, world, ts))
            if last is not None:
                last.close()
            last = r
            for _ in range(SPP):
                r.update()
            r.render()
            pad = L.rank_pixel_map(rank)[:, 0] < 0
            real = int((~pad).sum())
            for path in ("update", "batch"):
                if path == "batch":
                    r.reset_accumulation()
                    r.update_batch(SPP)
                for k, t in enumerate(tile_buffers(halart, r, L)):
                    # §9: padding tiles and the out-of-frame part of border tiles carry zeros (alpha included), as TileLayout.shard writes them
                    assert not t.cpu().numpy().reshape(-1, 4)[pad].view(np.uint32).any(), (path, rank, k)
                    if k < 3:
                        shards[path][k].append(t)
            st = r.statistics()
            assert st.rays_primary_total == real * SPP * 2, rank
            primary += st.rays_primary_total
            closest += st.rays_closest_total
            shadow += st.rays_shadow_total
        assert primary == w * h * SPP * 2
        assert (closest, shadow) == (rst.rays_closest_total, rst.rays_shadow_total)
        for path in ("update", "batch"):
            for k in range(3):
                gathered = torch.cat(shards[path][k]).contiguous()
                assert_same(L.unshard(gathered.cpu().numpy()), want[k], f"{path}: TileLayout.unshard of AOV {k}")
                last.scatter_gathered_tiles(k, gathered.data_ptr(), gathered.numel() * 4)
                assert_same(last.read_image(k), want[k], f"{path}: scatter_gathered_tiles of AOV {k}")
    finally:
        if last is not None:
            last.close()


@pytest.mark.parametrize("shard", [None, (2, 5, 12)], ids=["unsharded", "rank2-world5-ts12"])
def test_refused_tile_shards_leave_the_renderer_as_it_was(halart, shard):
    """hala_rt_set_tile_shard refuses tile_size 0 and 257, world 0 and rank >= world; afterwards the renderer renders the layout it
    had, bit for bit (the row-major image unsharded, the rank's tile buffers sharded)"""
    w, h = 61, 37
    L = TileLayout(w, h, shard[1], shard[2]) if shard else None
    r = renderer(halart, "cornell", w, h, shard=shard)
    try:
        def frame():
            r.reset_accumulation()
            r.update_batch(SPP)
            if shard is None:
                return [r.read_image(k).tobytes() for k in range(4)]
            return [t.cpu().numpy().tobytes() for t in tile_buffers(halart, r, L)]

        before = frame()
        for rank, world, ts, what in ((0, 4, 0, "tile size"), (0, 4, 257, "tile size"), (0, 0, 32, "rank / world"),
                                      (4, 4, 32, "rank / world"), (5, 5, 12, "rank / world")):
            with pytest.raises(halart.HalaRendererError, match=f"Invalid {what}"):
                r.set_tile_shard(rank, world, ts)
        assert frame() == before
    finally:
        r.close()
