"""Texel bundles (hala_rt_build_options::texture_bundles; RENDER_SPEC 7.4): the co-sized 8-bit maps of a material are also stored
interleaved and fetched together by the shade kernels.  The storage form must not be observable: with bundles on (the default) every image
equals the oracle's byte for byte and equals the render with bundles off; hala_rt_texture_bundle_info reports what was bundled, which
every case checks against a count made here from the scene alone (a case that bundled nothing would prove nothing)."""
import copy

import numpy as np
import pytest

import hala_renderer_amd as H
import scene_edits as E
from hala_renderer_amd import scenes, workloads
from hala_renderer_amd.scene import INVALID

gpu = pytest.mark.gpu
f32 = np.float32
IMAGES = {0: "accum", 1: "albedo", 2: "normal"}


# ---- what the library is expected to bundle, from the scene alone ---------------------------------------------------------------------------
def expected_bundles(scene):
    """-> (bundle count, bundled materials, textured but unbundled materials): a material is bundled when it references at least two
    maps and all of them are 8-bit images of equal width and height; materials that show the same tuple of images share a bundle"""
    nt = len(scene.texture2image_mapping)
    tuples, bundled, unbundled = set(), 0, 0
    for m in scene.materials:
        idx = (m.base_color_map_index, m.normal_map_index, m.metallic_roughness_map_index, m.emission_map_index)
        imgs = tuple(scene.image2data_mapping[scene.texture2image_mapping[t]] if t < nt else None for t in idx)
        used = [scene.image_data[i] for i in imgs if i is not None]
        if not used:
            continue
        same = all(d.format != scenes.A_FORMAT_FLOAT and (d.width, d.height) == (used[0].width, used[0].height) for d in used)
        if len(used) >= 2 and same:
            tuples.add(imgs)
            bundled += 1
        else:
            unbundled += 1
    return len(tuples), bundled, unbundled


def test_expected_bundles_counts():
    s = scenes.bunny_class(subdivisions=1, disney=True)
    assert expected_bundles(s) == (0, 0, 0)
    scenes.attach_textures(s, sets=1, size=8)
    assert expected_bundles(s) == (2, 2, 0)  # DISNEY: three maps, DIFFUSE: two of the same ones — different tuples
    s.materials[1].normal_map_index = INVALID
    assert expected_bundles(s) == (1, 1, 1)


def test_build_options_keep_their_size():
    import ctypes as C
    from hala_renderer_amd import _abi as A
    assert C.sizeof(A.BuildOptions) == 32 and A.BuildOptions.texture_bundles.offset == 20
    assert C.sizeof(A.TextureBundleInfo) == 24 and A.TextureBundleInfo.bundle_bytes.offset == 16


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def rand_image(fmt, w, h, seed, alpha=False):
    rng = np.random.RandomState(seed)
    if fmt == scenes.A_FORMAT_FLOAT:
        return H.HalaImageData(fmt, w, h, rng.rand(h, w, 4).astype(f32))
    px = (rng.rand(h, w, 4) * 255).astype(np.uint8)
    if not alpha:
        px[..., 3] = 255
    return H.HalaImageData(fmt, w, h, px)


def add_texture(s, img):
    k = len(s.image_data)
    s.image_data.append(img)
    t = len(s.texture2image_mapping)
    s.image2data_mapping[k] = k
    s.texture2image_mapping[t] = k
    return t


def blob_scene(size=32, w=48, h=36):
    """a Disney blob (material 0: base, normal, metallic-roughness) on a DIFFUSE ground (material 1: base, normal) under an env map"""
    s = scenes.bunny_class(subdivisions=3, aspect=w / h, disney=True)
    scenes.attach_textures(s, sets=1, size=size)
    kw = dict(width=w, height=h, max_depth=4, rr_depth=2, tonemap=(False, False, False), env_rotation=40.0, env_intensity=1.0, exposure=1.0)
    return s, scenes.sky_sun_envmap(64, 32, sun_gain=50.0), kw


def renderer(halart, scene, env, kw, bundles, build=None):
    r = halart.HalaRenderer("bundles", kw["width"], kw["height"], kw["max_depth"], kw["rr_depth"], *kw["tonemap"], 0)
    r.set_build_options(texture_bundles=bundles, **(build or {}))
    if env is not None:
        r.set_envmap(env, kw["env_rotation"])
        r.set_env_intensity(kw["env_intensity"])
    r.set_exposure_value(kw["exposure"])
    r.set_scene(scene)
    r.commit()
    return r


def oracle_images(oracle, scene, env, kw, frames):
    osc = oracle.OracleScene(scene, envmap=env)
    imgs, _ = osc.render(kw["width"], kw["height"], frames=frames, max_depth=kw["max_depth"], rr_depth=kw["rr_depth"], tonemap=kw["tonemap"],
                         env_rotation=kw["env_rotation"] if env is not None else 0.0, env_intensity=kw["env_intensity"] if env is not None else 1.0,
                         exposure=kw["exposure"])
    osc.close()
    return imgs


def info_tuple(r):
    i = r.texture_bundle_info()
    return i.bundle_count, i.bundled_materials, i.unbundled_textured_materials


def read(r):
    return {k: r.read_image(k) for k in IMAGES}


def assert_same(got, want, what):
    for k, name in IMAGES.items():
        if got[k].tobytes() != want[k].tobytes():
            bad = np.any(got[k].reshape(-1, 4) != want[k].reshape(-1, 4), axis=-1)
            raise AssertionError(f"{what}: {name}: {int(bad.sum())} of {bad.size} pixels differ")


def check(halart, oracle, scene, env, kw, what, frames=2, build=None, min_bundles=1):
    """bundles on == the oracle == bundles off, and the counts are the expected ones"""
    want_info = expected_bundles(scene)
    assert want_info[0] >= min_bundles, f"{what}: the case is expected to bundle something"
    want = oracle_images(oracle, scene, env, kw, frames)
    out = {}
    for bundles in (True, False):
        r = renderer(halart, scene, env, kw, bundles, build)
        try:
            info = info_tuple(r)
            if bundles:
                assert info == want_info, f"{what}: bundle info {info}, expected {want_info}"
                assert (r.texture_bundle_info().bundle_bytes > 0) == (want_info[0] > 0)
            else:
                assert info == (0, 0, want_info[1] + want_info[2]) and r.texture_bundle_info().bundle_bytes == 0
            r.update_batch(frames); r.render()
            out[bundles] = read(r)
        finally:
            r.close()
    assert_same(out[True], {k: want[k] for k in IMAGES}, f"{what}: bundles on vs the oracle")
    assert_same(out[True], out[False], f"{what}: bundles on vs off")


# ---- the scenes that are expected to bundle -----------------------------------------------------------------------------------------------
@gpu
def test_textured_atrium_slice(halart, oracle):
    s, env = workloads.atrium(target_triangles=120_000, aspect=16.0 / 9.0, texture_size=128)
    kw = dict(width=192, height=108, max_depth=workloads.MAX_DEPTH, rr_depth=workloads.RR_DEPTH, tonemap=(False, False, False), env_rotation=0.0,
              env_intensity=1.0, exposure=1.0)
    n_tex = sum(1 for m in s.materials if m.base_color_map_index != INVALID)
    assert n_tex >= 2 and expected_bundles(s)[1] == n_tex  # every textured material of the atrium is bundled
    check(halart, oracle, s, env, kw, "atrium")


@gpu
def test_cornell_box_with_textures(halart, oracle):
    from test_oracle_render import textured_scene
    s = textured_scene(size=64, fmt_variant=True)  # + a float emission map on material 1 and a 33 x 17 base map on material 2: those two stay unbundled
    b = expected_bundles(s)
    assert b[1] >= 2 and b[2] == 2
    check(halart, oracle, s, None, dict(width=72, height=72, max_depth=5, rr_depth=3, tonemap=(False, False, False), env_rotation=0.0, env_intensity=1.0,
                                        exposure=1.0), "textured cornell", frames=3)


# ---- fallbacks and corner cases ------------------------------------------------------------------------------------------------------------
def case_sizes_differ():
    s, env, kw = blob_scene()
    s.materials[0].normal_map_index = add_texture(s, rand_image(scenes.A_FORMAT_UNORM, 16, 16, 1))
    return s, env, kw, (1, 1, 1)


def case_float_map():
    s, env, kw = blob_scene()
    s.materials[0].metallic_roughness_map_index = add_texture(s, rand_image(scenes.A_FORMAT_FLOAT, 32, 32, 2))
    return s, env, kw, (1, 1, 1)


def case_single_map():
    s, env, kw = blob_scene()
    s.materials[1].normal_map_index = INVALID
    return s, env, kw, (1, 1, 1)


def case_shared_map_different_partners():
    s, env, kw = blob_scene()
    s.materials[0].metallic_roughness_map_index = INVALID  # material 0: (base 0, normal 1), material 1: (base 0, another normal map)
    s.materials[1].normal_map_index = add_texture(s, rand_image(scenes.A_FORMAT_UNORM, 32, 32, 3))
    return s, env, kw, (2, 2, 0)


def case_emission_map():
    s, env, kw = blob_scene()
    s.materials[0].emission = (1.0, 0.8, 0.6)
    s.materials[0].emission_map_index = add_texture(s, rand_image(scenes.A_FORMAT_SRGB, 32, 32, 4))  # all four lanes
    s.materials[1].emission = (0.5, 0.5, 0.5)
    s.materials[1].normal_map_index = INVALID
    s.materials[1].emission_map_index = 0  # base + emission only: lanes 0 and 3
    return s, env, kw, (2, 2, 0)


def case_odd_sizes():
    s, env, kw = blob_scene(size=33)
    return s, env, kw, (2, 2, 0)


def case_non_square_odd():
    s, env, kw = blob_scene()
    for m in s.materials:
        m.base_color_map_index = m.normal_map_index = m.metallic_roughness_map_index = INVALID
    t = [add_texture(s, rand_image(f, 37, 10, 10 + k)) for k, f in enumerate((scenes.A_FORMAT_SRGB, scenes.A_FORMAT_UNORM, scenes.A_FORMAT_UNORM))]
    s.materials[0].base_color_map_index, s.materials[0].normal_map_index, s.materials[0].metallic_roughness_map_index = t
    s.materials[1].base_color_map_index, s.materials[1].metallic_roughness_map_index = t[0], t[2]
    return s, env, kw, (2, 2, 0)


def case_top_mip():
    """2 x 2 maps seen from afar: the level of detail ends on the 1 x 1 top level (and between the two levels on the way there)"""
    s, env, kw = blob_scene()
    for m in s.materials:
        m.base_color_map_index = m.normal_map_index = m.metallic_roughness_map_index = INVALID
    a = add_texture(s, rand_image(scenes.A_FORMAT_SRGB, 2, 2, 20))
    b = add_texture(s, rand_image(scenes.A_FORMAT_UNORM, 2, 2, 21))
    c = add_texture(s, rand_image(scenes.A_FORMAT_SRGB, 1, 1, 22))
    d = add_texture(s, rand_image(scenes.A_FORMAT_UNORM, 1, 1, 23))
    s.materials[0].base_color_map_index, s.materials[0].metallic_roughness_map_index = a, b
    s.materials[1].base_color_map_index, s.materials[1].normal_map_index = c, d  # a chain of one level
    return s, env, kw, (2, 2, 0)


def case_translucent_base_map():
    """a cut-out base map with alpha next to a normal map: bundled for shading, while the any-hit rays keep reading the map's own arena"""
    s, env, kw = blob_scene()
    s.materials[0].base_color_map_index = add_texture(s, E._alpha_checker(32))
    s.materials[1].base_color_map_index = add_texture(s, rand_image(scenes.A_FORMAT_SRGB, 32, 32, 5, alpha=True))
    return s, env, kw, (2, 2, 0)


CASES = {f.__name__[5:]: f for f in (case_sizes_differ, case_float_map, case_single_map, case_shared_map_different_partners, case_emission_map,
                                     case_odd_sizes, case_non_square_odd, case_top_mip, case_translucent_base_map)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_are_what_they_claim(name):
    s, _, _, counts = CASES[name]()
    assert expected_bundles(s) == counts


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fallbacks_and_corner_cases(halart, oracle, name):
    s, env, kw, counts = CASES[name]()
    assert expected_bundles(s) == counts
    check(halart, oracle, s, env, kw, name, frames=3)


@gpu
def test_no_texture_no_bundle(halart):
    s = scenes.cornell_box()
    r = renderer(halart, s, None, dict(width=32, height=32, max_depth=3, rr_depth=2, tonemap=(False, False, False), exposure=1.0), True)
    try:
        i = r.texture_bundle_info()
        assert (i.bundle_count, i.bundled_materials, i.unbundled_textured_materials, i.bundle_bytes) == (0, 0, 0, 0)
    finally:
        r.close()


@gpu
def test_bundle_info_needs_a_commit_and_options_are_checked(halart):
    r = halart.HalaRenderer("bundles", 16, 16, 2, 1, False, False, False, 0)
    try:
        with pytest.raises(halart.HalaRendererError):
            r.texture_bundle_info()
        o = halart._abi.BuildOptions(texture_bundles=2)
        assert r._lib.hala_rt_set_build_options(r._h, o) != 0
    finally:
        r.close()


# ---- edits ---------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_map_indices_edited_then_refit(halart, oracle):
    """hala_rt_update_material + hala_rt_refit: the table follows new map indices — onto a tuple that needs a new bundle, off the bundles
    (one map left), and back — each time bit-exact against a fresh commit of the edited scene and against the oracle"""
    s, env, kw = blob_scene()
    extra_nrm = add_texture(s, rand_image(scenes.A_FORMAT_UNORM, 32, 32, 30))
    small = add_texture(s, rand_image(scenes.A_FORMAT_SRGB, 16, 16, 31))
    steps = [
        ("new tuple", {0: dict(normal_map_index=extra_nrm)}),
        ("one map left", {0: dict(normal_map_index=INVALID, metallic_roughness_map_index=INVALID)}),
        ("sizes differ", {1: dict(base_color_map_index=small)}),
        ("back", {0: dict(normal_map_index=1, metallic_roughness_map_index=2), 1: dict(base_color_map_index=0)}),
    ]
    r = renderer(halart, s, env, kw, True)
    try:
        assert info_tuple(r) == expected_bundles(s) == (2, 2, 0)
        r.update_batch(2); r.render()
        edited = copy.deepcopy(s)
        for what, changes in steps:
            for k, ch in changes.items():
                for field, v in ch.items():
                    setattr(edited.materials[k], field, v)
                r.update_material(k, edited.materials[k])
            r.refit()
            want_info = expected_bundles(edited)
            got_info = info_tuple(r)
            assert got_info[1:] == want_info[1:], (what, got_info, want_info)
            assert got_info[0] >= want_info[0], (what, got_info, want_info)  # bundles no longer referenced may stay until the next commit
            r.update_batch(2); r.render()
            got = read(r)
            assert_same(got, oracle_images(oracle, edited, env, kw, 2), f"{what}: refit vs the oracle")
            fresh = renderer(halart, copy.deepcopy(edited), env, kw, True)
            try:
                assert info_tuple(fresh) == want_info, what
                fresh.update_batch(2); fresh.render()
                assert_same(got, read(fresh), f"{what}: refit vs a fresh commit")
            finally:
                fresh.close()
    finally:
        r.close()


@gpu
def test_two_level_tree_with_bundles(halart, oracle):
    """RENDER_SPEC 4.5: shading records are found through the instance; the bundle is found through the material all the same"""
    s, env, kw = blob_scene()
    s.nodes.append(H.HalaNode(name="blob_copy", mesh_index=0, local_transform=E._translate((1.6, 0.2, -1.0)) @ E._rot(ry=0.7) @ E._scale((0.6, 0.6, 0.6))))
    s.nodes.append(H.HalaNode(name="blob_copy_2", mesh_index=0, local_transform=E._translate((-1.7, 0.0, -0.5)) @ E._rot(rx=0.4)))
    oracle.set_instancing(True)
    try:
        r = renderer(halart, s, env, kw, True, build=dict(instancing=True))
        try:
            assert r.bvh_info().instance_ref_count > 0
        finally:
            r.close()
        check(halart, oracle, s, env, kw, "two-level", build=dict(instancing=True))
    finally:
        oracle.set_instancing(False)
