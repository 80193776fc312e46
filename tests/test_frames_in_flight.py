"""Two updates in flight (hala_rt_set_frames_in_flight): untimed updates alternate between two frame slots, each with its
own stream, control block, spill area, per-path state and queues; only the resolve and the Cryptomatte fold stay in frame order.  On the
GPU tier: every sequence of calls gives, byte for byte, what the same sequence gives with one slot (set_frames_in_flight(1)), and the
plain sequence gives what the oracle gives.  Every comparison is tobytes() equality.

Scene: workloads.atrium(20 000 triangles, 64 x 64 textures) under its environment map at 97 x 55, max_depth 5, rr_depth 3 — a tree that
is not staged in LDS (the large-scene traversal kernels, the kind sort of the bounce queues and the texel bundles run), a frame that is no
multiple of the 8 x 8 pixel block: 13 x 7 blocks = 5 824 path slots per sample, 5 335 of them real; at 3 samples per pass 17 472 slots,
which end inside a sort window.  A Cornell box at 67 x 45 covers the LDS-staged traversal and the SIMPLE shade variants, whose updates
alternate between the two streams but share one set of buffers.

Bounce launches of k_shade / k_shade_sort that walk the queue with a grid stride were built and measured 40 % slower
(profiles/frames_in_flight.txt, section 8) and are not part of the library, so they have no case here."""
import functools

import numpy as np
import pytest

from hala_renderer_amd import dist, scenes, workloads
from hala_renderer_amd.scene import INVALID

gpu = pytest.mark.gpu
W, H = 97, 55
MAX_DEPTH, RR_DEPTH = 5, 3
TOTALS = ("total_frames", "updates_rendered", "rays_total", "rays_closest_total", "rays_shadow_total", "rays_primary_total")


@functools.lru_cache(maxsize=None)
def atrium():
    return workloads.atrium(target_triangles=20_000, aspect=W / H, texture_size=64)


def make(halart, which="atrium", in_flight=2, setup=None):
    if which == "atrium":
        scene, env = atrium()
        w, h = W, H
    else:
        scene, env, w, h = scenes.cornell_box(aspect=67 / 45), None, 67, 45
    r = halart.HalaRenderer("in_flight", w, h, MAX_DEPTH, RR_DEPTH, False, False, False, 0)
    try:
        if env is not None:
            r.set_envmap(env, 0.0)
        r.set_scene(scene)
        r.commit()
        assert (r.bvh_info().lds_node_count == 0) == (which == "atrium")
        r.set_launch_timing_period(0)
        r.set_frames_in_flight(in_flight)
        if setup is not None:
            setup(r)
    except Exception:
        r.close()
        raise
    return r


def images(r, n=4, view=0):
    return [r.read_image(k, view=view) for k in range(n)]


def totals(r):
    s = r.statistics()
    return np.array([getattr(s, f) for f in TOTALS], dtype=np.uint64)


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, i)
        assert a.tobytes() == b.tobytes(), f"{what}: item {i} differs in {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes"


def both(halart, script, which="atrium", setup=None, used=None):
    """script(r) -> list of arrays; run with two slots and with one.  used: filled with frames_in_flight_info() of the two runs"""
    out = []
    for n in (2, 1):
        r = make(halart, which, n, setup)
        try:
            out.append(script(r))
            if used is not None:
                used.append(r.frames_in_flight_info())
        finally:
            r.close()
    same(out[0], out[1], "two slots against one")
    return out[0]


# ---- case 1: in flight against serial against the oracle ---------------------------------------------------------------------------
def six_updates(r):
    for _ in range(6):
        r.update()
    return images(r) + [totals(r)]


@gpu
@pytest.mark.parametrize("which", ["atrium", "cornell"])
def test_six_updates_in_flight(halart, oracle, which):
    used = []
    got = both(halart, six_updates, which, used=used)
    # two slots: updates ran on the second one — with its own buffers on the large tree (allocated when the second update found the first
    # still running: a 12-launch update outlasts the host's enqueueing of the next), on slot 0's buffers on the LDS-staged tree; one slot: none
    assert used[0][0] >= 1 and used[0][1] == (which == "atrium"), used
    assert used[1] == (0, False), used
    if which == "atrium":
        scene, env = atrium()
        w, h = W, H
    else:
        scene, env, w, h = scenes.cornell_box(aspect=67 / 45), None, 67, 45
    want, ost = oracle.OracleScene(scene, envmap=env).render(w, h, frames=6, max_depth=MAX_DEPTH, rr_depth=RR_DEPTH)
    same(got[:4], want, f"{which}: against the oracle")
    t = dict(zip(TOTALS, got[4].tolist()))
    assert (t["rays_closest_total"], t["rays_shadow_total"]) == (ost.rays_closest, ost.rays_shadow)


# ---- case 2: interleavings ------------------------------------------------------------------------------------------------------------
def grow_the_batch(r):
    r.update_batch(3); r.update(); r.update_batch(2)
    return images(r) + [totals(r)]


def restart_between(r):
    r.update(); r.update(); r.reset_accumulation(); r.update(); r.update_batch(2)
    return images(r) + [totals(r)]


def timed_and_untimed(r):
    r.set_launch_timing_period(2)
    for _ in range(5):
        r.update()
    return images(r) + [totals(r)]


def counting_in_the_middle(r):
    r.update(); r.update()
    r.set_counting(True); r.update(); r.set_counting(False)
    r.update(); r.update()
    s = r.statistics()
    return images(r) + [totals(r), np.array([s.nodes_closest_total, s.tris_closest_total, s.nodes_shadow_total, s.tris_shadow_total], dtype=np.uint64)]


def readers_between(r):
    out = []
    for _ in range(3):
        r.update(); r.update()
        out.append(totals(r))
        r.update()
        out += images(r)
    return out


def refit_between(r):
    scene, _ = atrium()
    node = next(i for i, nd in enumerate(scene.nodes) if nd.mesh_index != INVALID)
    m = np.array(scene.nodes[node].local_transform, dtype=np.float32)
    m[1, 3] += 0.125
    r.update(); r.update()
    r.update_node_transform(node, m)
    r.update()
    r.refit()
    r.update(); r.update(); r.update()
    return images(r) + [totals(r)]


def toggled(r):
    r.update(); r.update()
    r.set_frames_in_flight(1)
    r.update(); r.update()
    r.set_frames_in_flight(2)
    r.update(); r.update(); r.update()
    return images(r) + [totals(r)]


INTERLEAVINGS = {"grow_the_batch": grow_the_batch, "restart_between": restart_between, "timed_and_untimed": timed_and_untimed,
                 "counting_in_the_middle": counting_in_the_middle, "readers_between": readers_between, "refit_between": refit_between,
                 "toggled": toggled}


@gpu
@pytest.mark.parametrize("name", sorted(INTERLEAVINGS))
def test_interleavings(halart, name):
    both(halart, INTERLEAVINGS[name])


@gpu
@pytest.mark.parametrize("which", ["atrium", "cornell"])
def test_close_with_two_updates_in_flight(halart, which):
    r = make(halart, which)
    r.update_batch(4); r.update_batch(4)
    r.close()
    r = make(halart, which)  # the device is still usable
    try:
        r.update()
        assert np.isfinite(r.read_image(0)).all()
    finally:
        r.close()


# ---- case 3: features on ----------------------------------------------------------------------------------------------------------------
def plain(r):
    for frames in (1, 2, 1, 1):
        r.update_batch(frames)
    return images(r) + [totals(r)]


def adaptive(r):
    r.set_adaptive_sampling(0.05, min_samples=2, interval=2)  # snapshot at frame 1, checks from frame 2 on
    for frames in (1, 1, 2, 1, 1, 3):
        r.update_batch(frames)
    st = r.adaptive_status()
    return images(r) + [r.read_sample_counts(), np.array([st.active_blocks, st.active_pixels, st.samples, st.last_snapshot], dtype=np.uint64), totals(r)]


def light_groups(r):
    r.set_light_groups(environment=1)
    out = plain(r)
    return out + [r.read_light_group(g) for g in range(r.light_group_count)]


def aovs_and_cryptomatte(r):
    r.set_aovs(position=True, ids=True)
    r.set_cryptomatte()
    out = plain(r)
    return out + [r.read_image(4), r.read_image(5)] + [r.read_cryptomatte_records(layer) for layer in ("object", "material", "asset")]


def two_views(r):
    r.set_views([0, 0])
    out = plain(r)
    return out + images(r, view=1)


FEATURES = {"adaptive": adaptive, "light_groups": light_groups, "aovs_and_cryptomatte": aovs_and_cryptomatte, "two_views": two_views}


@gpu
@pytest.mark.parametrize("name", sorted(FEATURES))
def test_features_in_flight(halart, name):
    both(halart, FEATURES[name])


# ---- case 4: what a path slot holds changes while slot 1 owns buffers ----------------------------------------------------------------
def shape_changes(r):
    """five segments, each behind a setter that restarts the accumulation: the per-path arrays grow and shrink (AOVs, light groups, the
    Cryptomatte first-hit records, the batch capacity) while the second slot is already sized for what came before"""
    crypto = lambda: [r.read_cryptomatte_records(layer) for layer in ("object", "material", "asset")]
    groups = lambda: [r.read_light_group(g) for g in range(r.light_group_count)]
    out = []
    for _ in range(3):
        r.update()
    out += images(r) + [totals(r)]
    r.set_aovs(position=True, ids=True)
    for _ in range(3):
        r.update()
    out += images(r, 6) + [totals(r)]
    r.set_light_groups(environment=1)
    r.update_batch(3); r.update(); r.update()  # the batch grows the capacity while slot 1 is sized
    out += images(r, 6) + groups() + [totals(r)]
    r.set_aovs(position=False, ids=False)
    r.set_cryptomatte()
    for _ in range(3):
        r.update()
    out += images(r) + groups() + crypto() + [totals(r)]
    r.set_light_groups()
    r.update_batch(2); r.update()
    return out + crypto() + [totals(r)] + images(r)  # last: three frames, images 0-3 as with every feature off


@gpu
@pytest.mark.parametrize("which", ["atrium", "cornell"])
def test_shape_changes_in_flight(halart, oracle, which):
    used = []
    got = both(halart, shape_changes, which, used=used)
    assert used[0][0] >= 1 and used[0][1] == (which == "atrium"), used
    assert used[1] == (0, False), used
    if which == "atrium":
        scene, env = atrium()
        w, h = W, H
    else:
        scene, env, w, h = scenes.cornell_box(aspect=67 / 45), None, 67, 45
    want, _ = oracle.OracleScene(scene, envmap=env).render(w, h, frames=3, max_depth=MAX_DEPTH, rr_depth=RR_DEPTH)
    same(got[-4:], want, f"{which}: the last segment against the oracle")


@gpu
def test_tile_shard_in_flight(halart):
    """two emulated ranks of a 2-rank shard, 16 x 16 tiles: each rank's tile buffers with two slots against one"""
    import torch

    def tiles(r):
        for frames in (1, 2, 1, 1):
            r.update_batch(frames)
        r.wait_idle()
        out = []
        for k in range(3):
            ptr, nbytes = r.tile_buffer(k)
            out.append(torch.as_tensor(dist._DeviceView(ptr, nbytes // 4), device="cuda:0").clone().cpu().numpy())
        return out + [totals(r)]

    for rank in range(2):
        both(halart, tiles, setup=lambda r, rank=rank: r.set_tile_shard(rank, 2, 16))

