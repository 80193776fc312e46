"""The scratch contract of the query batches, across all kinds together.  Every device form — ray batch, multi-hit, closest points,
distance grid, occlusion, bake map, bake atlas — runs on the caller's stream, ordered behind the previous user of the renderer's scratch
(work counters, spill area, the re-based rays, the grid's row bits, the mask words, the bake buffers), without a host synchronisation, and
leaves an event for the next user.  The per-kind test files run each kind alone on a second stream; here the kinds follow one another,
alternating between the renderer's stream and a side stream, with nothing in between but what the library queues itself.

The reference of every call is the same call made alone on a fresh renderer, and of the frame that follows, a renderer that made no
queries: equality is of bytes, so no tolerance is involved.  Shapes are the smallest at which the shared state is in play: 256 rays
(k = 4), 256 point queries, a signed 8 x 8 x 8 grid (the row pass and the distance pass both use the work counters), 64 occlusion samples
x 33 rays (two mask words a sample, kept in the renderer's own mask buffer), 16 x 16 maps x 16 rays (an atlas of two instances)."""
import numpy as np
import pytest

import hala_renderer_amd as H
import test_bake as TB
from test_bake import BIAS, REACH, SEED

A = H._abi
gpu = pytest.mark.gpu
f32 = np.float32
N, K, GRID, SAMPLES, AO_RAYS, MAP, MAP_RAYS = 256, 4, 8, 64, 33, 16, 16
CHARTS = ((6, (0.5, 0.5), (0.0, 0.0), True, False), (7, (0.25, 0.5), (0.625, 0.25), False, True))
KINDS = ("rays", "multi", "points", "grid", "occlusion", "bake", "atlas")
# output buffers of a kind, in bytes
OUT_BYTES = {"rays": (N * 16,), "multi": (N * K * 16, N * 4), "points": (N * 32,), "grid": (GRID ** 3 * 4, GRID ** 3 * 4), "occlusion": (SAMPLES * 16,),
             "bake": (MAP * MAP * 16, MAP * MAP * 16), "atlas": (MAP * MAP * 16, MAP * MAP * 16)}


def carpets():
    return TB.in_cornell(TB.chart(8), extra=TB.chart(4))[0]


def host_inputs():
    """rays and points inside the Cornell box (555 units wide), in every direction"""
    rng = np.random.RandomState(7)
    d = rng.normal(size=(N, 3))
    rays = np.zeros(N, dtype=A.RAY_DTYPE)
    rays["origin"] = rng.uniform(20.0, 535.0, size=(N, 3))
    rays["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays["tmax"] = np.inf
    points = np.zeros(N, dtype=A.POINT_QUERY_DTYPE)
    points["point"] = rng.uniform(-50.0, 600.0, size=(N, 3))
    points["radius"] = np.inf
    nrm = rng.normal(size=(SAMPLES, 3))
    samples = np.zeros(SAMPLES, dtype=A.OCCLUSION_SAMPLE_DTYPE)
    samples["point"] = rng.uniform(20.0, 535.0, size=(SAMPLES, 3))
    samples["normal"] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    samples["bias"] = BIAS
    samples["reach"] = REACH
    return dict(rays=rays, points=points, samples=samples)


def call(r, kind, d_in, out, stream):
    """the device form of `kind` on `stream` (0: the renderer's own) into the tensors `out`"""
    if kind == "rays":
        r.trace_rays(d_in["rays"].data_ptr(), out[0].data_ptr(), N, 0, 0, stream)
    elif kind == "multi":
        r.trace_rays_multi(d_in["rays"].data_ptr(), out[0].data_ptr(), N, K, out[1].data_ptr(), stream)
    elif kind == "points":
        assert r.closest_points(d_in["points"], out=out[0], stream=stream) is None
    elif kind == "grid":
        assert r.distance_grid((30.0, 30.0, 30.0), 70.0, (GRID, GRID, GRID), signed=True, out=out[0], out_prim=out[1], stream=stream) is None
    elif kind == "occlusion":
        assert r.occlusion(d_in["samples"], rays=AO_RAYS, seed=SEED, out=out[0], stream=stream) is None
    elif kind == "bake":
        assert r.bake_occlusion(6, MAP, MAP, MAP_RAYS, SEED, margin=2, bias=BIAS, reach=REACH, out=out[0], out_texels=out[1], stream=stream) is None
    else:
        assert r.bake_atlas_occlusion(CHARTS, MAP, MAP, MAP_RAYS, SEED, margin=2, bias=BIAS, reach=REACH, out=out[0], out_texels=out[1], stream=stream) is None


def device_buffers(torch, host):
    d_in = {name: torch.from_numpy(a.view(np.uint8).copy()).cuda() for name, a in host.items()}
    out = {kind: tuple(torch.zeros(n, dtype=torch.uint8, device="cuda") for n in OUT_BYTES[kind]) for kind in KINDS}
    torch.cuda.synchronize()
    return d_in, out


@pytest.fixture(scope="module")
def alone(halart):
    """every call alone on a fresh renderer, and the frame of a renderer that made no queries: computed once, left unchanged"""
    import torch
    from test_gpu_parity import make_renderer
    scene, host, want = carpets(), host_inputs(), {}
    for kind in KINDS:
        r = make_renderer(halart, scene, 32, 32)
        d_in, out = device_buffers(torch, host)
        call(r, kind, d_in, out[kind], 0)
        r.wait_idle()
        want[kind] = tuple(t.cpu().numpy().tobytes() for t in out[kind])
        r.close()
        assert all(any(b) for b in want[kind]), f"{kind}: an output is still its prefill"
    hits = np.frombuffer(want["rays"][0], dtype=A.HIT_DTYPE)
    counts = np.frombuffer(want["multi"][1], dtype=np.uint32)
    vis = np.frombuffer(want["occlusion"][0], dtype=A.OCCLUSION_DTYPE)["visibility"]
    grid = np.frombuffer(want["grid"][0], dtype=f32)
    baked = np.frombuffer(want["atlas"][1], dtype=A.BAKE_TEXEL_DTYPE)["prim"] != 0xFFFFFFFF
    assert (hits["prim"] != 0xFFFFFFFF).sum() > N // 2 and counts.max() > 1, "the rays hit, and more than once"
    assert (vis > 0).any() and (vis < 1).any() and (grid < 0).any() and (grid > 0).any() and baked.any() and not baked.all(), "the inputs are telling"
    r = make_renderer(halart, scene, 32, 32)
    r.update(); r.render()
    frame = [r.read_image(which).tobytes() for which in range(4)]
    r.close()
    return scene, host, want, frame


@gpu
@pytest.mark.parametrize("first_on_side", [False, True], ids=["renderer-stream-first", "side-stream-first"])
def test_all_kinds_alternating_between_two_streams(halart, alone, first_on_side):
    """seven device forms back to back, every other one on the side stream, no host synchronisation between them; then one; then a frame"""
    import torch
    from test_gpu_parity import make_renderer
    scene, host, want, frame = alone
    r = make_renderer(halart, scene, 32, 32)
    d_in, out = device_buffers(torch, host)
    side = torch.cuda.Stream()
    for i, kind in enumerate(KINDS):
        call(r, kind, d_in, out[kind], side.cuda_stream if (i % 2 == 1) != first_on_side else 0)
    torch.cuda.synchronize()
    for kind in KINDS:
        got = tuple(t.cpu().numpy().tobytes() for t in out[kind])
        for j, (g, w) in enumerate(zip(got, want[kind])):
            assert g == w, f"{kind}: output {j} differs from the call made alone"
    r.update(); r.render()
    assert [r.read_image(which).tobytes() for which in range(4)] == frame, "the frame after the queries"
    r.close()
