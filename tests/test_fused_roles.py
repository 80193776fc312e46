"""The fused traversal launch (csrc/trace_shadow.hip: k_trace_shadow_then_batch) against frames with one launch per pass and against the
oracle, bit for bit — no tolerances anywhere.

A workgroup of the fused launch starts on one of the launch's three queues (light connections, environment connections, the next bounce's
closest-hit rays) and visits the others afterwards; which one it starts on follows from the queue sizes.  Nothing a frame computes may
depend on that: every case renders the same frames with fused launches and with one launch per pass and compares all four images and
the ray totals, whatever the proportions are — with every queue there, with a queue absent, with only the last bounce's launch, with
queues far smaller than the grid, with light groups, with one and two frames in flight, on the large-scene and on the LDS-staged kernels."""
import pytest

from hala_renderer_amd import scenes
from hala_renderer_amd.scene import INVALID
from test_gpu_parity import make_renderer
from test_traversal_paths import assert_large

gpu = pytest.mark.gpu
FUSED_FAMILY = 3  # _abi.VARIANT_FAMILIES: k_trace_shadow_then_batch, flags (ALPHA, STAGED, INST, GROUPS) from bit 0
STAGED_BIT, GROUPS_BIT = 1, 3
FRAMES = 2

_SCENES = {}


def scene_of(name):
    """sponza: the 60 k-triangle atrium with its two quad lights; sponza_unlit: the same without them; cornell: the Cornell box (LDS-staged)"""
    if name not in _SCENES:
        if name == "cornell":
            s = scenes.cornell_box(aspect=64 / 36)
        else:
            s = scenes.sponza_class(target_triangles=60000, disney=False)
            if name == "sponza_unlit":
                s.nodes = [nd for nd in s.nodes if nd.light_index == INVALID]  # the light nodes are leaves at the end of the list
                s.lights = []
        _SCENES[name] = s
    return _SCENES[name]


_ENV = []


def sky():
    if not _ENV:
        _ENV.append(scenes.sky_sun_envmap(128, 64, sun_gain=300.0))
    return _ENV[0]


_WANT = {}


def oracle_images(oracle, scene, env, w, h, max_depth, rr_depth):
    key = (scene, env, w, h, max_depth, rr_depth)
    if key not in _WANT:
        want, _ = oracle.OracleScene(scene_of(scene), envmap=sky() if env else None).render(w, h, frames=FRAMES, max_depth=max_depth, rr_depth=rr_depth)
        _WANT[key] = [x.tobytes() for x in want]
    return _WANT[key]


def render(halart, scene, env, w, h, max_depth, rr_depth, fusion, in_flight=None, groups=False):
    """(the four images, the light-group images, rays_total, the fused family's launched mask) of FRAMES frames"""
    s = scene_of(scene)
    halart.variant_ledger(FUSED_FAMILY, reset=True)
    r = make_renderer(halart, s, w, h, max_depth=max_depth, rr_depth=rr_depth, env=sky() if env else None, build=dict(instancing=False))
    try:
        if scene == "cornell":
            assert r.bvh_info().lds_node_count > 0
        else:
            assert_large(r)
        r.set_pass_fusion(fusion)
        if groups:
            r.set_light_groups(lights=[k % 2 for k in range(len(s.lights))], environment=1, materials=2)
        if in_flight is None:
            r.update_batch(FRAMES)
        else:  # separate updates: with two in flight the second starts beside the first's last launches
            r.set_frames_in_flight(in_flight)
            for _ in range(FRAMES):
                r.update()
        r.render()
        images = [r.read_image(k).tobytes() for k in range(4)]
        group_images = [r.read_light_group(g).tobytes() for g in range(3)] if groups else []
        rays = r.statistics().rays_total
    finally:
        r.close()
    return images, group_images, rays, halart.variant_ledger(FUSED_FAMILY, reset=True)[0]


CASES = {
    # name: (scene, environment map, width, height, max_depth, rr_depth, frames in flight, light groups)
    "lights_and_env": ("sponza", True, 64, 36, 5, 3, None, False),        # the full three-queue launch
    "env_only": ("sponza_unlit", True, 64, 36, 5, 3, None, False),        # no light: the light queue does not exist
    "light_only": ("sponza", False, 64, 36, 5, 3, None, False),           # no environment: the environment queue does not exist
    "max_depth_1": ("sponza", True, 64, 36, 1, 3, None, False),           # only the last bounce's launch: two shadow queues, no closest-hit pass
    "max_depth_2": ("sponza", True, 64, 36, 2, 3, None, False),
    "frame_8x8": ("sponza", True, 8, 8, 5, 3, None, False),               # queues far smaller than a shard and than the grid: most workgroups find everything dry
    "light_groups": ("sponza", True, 64, 36, 5, 3, None, True),           # the GROUPS variant
    "in_flight_1": ("sponza", True, 64, 36, 5, 3, 1, False),
    "in_flight_2": ("sponza", True, 64, 36, 5, 3, 2, False),
    "cornell_lights_and_env": ("cornell", True, 64, 36, 5, 3, None, False),  # the LDS-staged variants
}


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_fused_launches_equal_per_pass_frames_and_the_oracle(halart, oracle, case):
    scene, env, w, h, max_depth, rr_depth, in_flight, groups = CASES[case]
    want = oracle_images(oracle, scene, env, w, h, max_depth, rr_depth)
    fused = render(halart, scene, env, w, h, max_depth, rr_depth, 2, in_flight, groups)
    per_pass = render(halart, scene, env, w, h, max_depth, rr_depth, 0, in_flight, groups)
    # the fused symbol ran, in the variant the case is about, and only where it was asked for
    assert per_pass[3] == 0
    assert fused[3] != 0
    for bit in range(16):
        if (fused[3] >> bit) & 1:
            assert ((bit >> STAGED_BIT) & 1) == (scene == "cornell"), bit
    if groups:
        assert any((fused[3] >> bit) & 1 and (bit >> GROUPS_BIT) & 1 for bit in range(16))
    for k in range(4):
        assert fused[0][k] == per_pass[0][k], f"image {k}: fused launches differ from one launch per pass"
        assert fused[0][k] == want[k], f"image {k}: fused launches differ from the oracle"
        assert per_pass[0][k] == want[k], f"image {k}: one launch per pass differs from the oracle"
    assert fused[1] == per_pass[1], "light-group images"
    assert fused[2] == per_pass[2] and fused[2] > 0, "rays_total"
