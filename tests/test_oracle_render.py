"""CPU tier: the oracle's traversal + integrator (docs/RENDER_SPEC.md).  Pixel parity with the reference is UNPINNED
(its shaders are not in the repository); what is pinned here is internal consistency — BVH traversal vs a
brute-force intersector, analytic renders, frozen regression fixtures — so that the oracle can act as the spec the HIP
kernels are held to in tests/test_gpu_parity.py."""
import os
import sys

import numpy as np
import pytest

import first_hit_ref
import hala_renderer_amd as H
from conftest import GOLDEN
from hala_renderer_amd import scenes

f32 = np.float32


def random_rays(n, lo, hi, seed):
    rng = np.random.RandomState(seed)
    rays = np.zeros(n, dtype=H._abi.RAY_DTYPE)
    rays["origin"] = (lo + rng.rand(n, 3) * (hi - lo)).astype(f32)
    d = rng.randn(n, 3)
    rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    rays["tmin"] = 0.0
    rays["tmax"] = np.where(rng.rand(n) < 0.3, rng.rand(n) * np.linalg.norm(hi - lo), 3.0e38).astype(f32)
    return rays


@pytest.mark.parametrize("scene_name", ["cornell", "blob", "sponza_small", "single_tri"])
def test_bvh_traversal_equals_brute_force(oracle, scene_name):
    if scene_name == "cornell":
        s = scenes.cornell_box()
    elif scene_name == "blob":
        s = scenes.bunny_class(subdivisions=2)
    elif scene_name == "sponza_small":
        s = scenes.sponza_class(target_triangles=3000)
    else:
        s = scenes.cornell_box()
        s.meshes = [H.HalaMesh([H.HalaPrimitive(indices=np.array([0, 1, 2], np.uint32), vertices=s.meshes[0].primitives[0].vertices[:3], material_index=0)])]
        s.nodes = [H.HalaNode(name="t", mesh_index=0), s.nodes[3]]
    osc = oracle.OracleScene(s)
    mn, mx = osc.bounds()
    pad = (mx - mn) * 0.3 + 1e-3
    rays = random_rays(4000, mn - pad, mx + pad, 5)
    for mode in (0, 1):
        a = osc.trace(rays, mode)
        b = osc.trace(rays, mode, brute=True)
        if mode == 0:
            assert np.array_equal(a["prim"], b["prim"])
            assert a["t"].tobytes() == b["t"].tobytes() and a["u"].tobytes() == b["u"].tobytes() and a["v"].tobytes() == b["v"].tobytes()
        else:
            assert np.array_equal(a["t"], b["t"])


def test_closest_hit_tie_break_prefers_lower_id(oracle):
    """two coincident triangles: RENDER_SPEC §4.2 says equal t -> lower global id, independent of BVH order"""
    s = scenes.cornell_box()
    prim = s.meshes[0].primitives[0]
    tri = H.HalaPrimitive(indices=np.array([0, 1, 2, 0, 1, 2], np.uint32), vertices=prim.vertices[:3].copy(), material_index=0)
    s.meshes = [H.HalaMesh([tri])]
    s.nodes = [H.HalaNode(name="t", mesh_index=0), s.nodes[3]]
    osc = oracle.OracleScene(s)
    v = prim.vertices[:3]["position"]
    c = v.mean(axis=0)
    rays = np.zeros(1, dtype=H._abi.RAY_DTYPE)
    rays["origin"] = c + np.array([0, 100.0, 0], dtype=f32); rays["direction"] = (0, -1, 0); rays["tmax"] = 1e30
    h = osc.trace(rays, 0)
    assert h["prim"][0] == 0 and h["t"][0] > 0


def test_primary_hit_table_fixture(oracle):
    g = np.load(os.path.join(GOLDEN, "cornell_primary_hits_16x16.npz"))
    osc = oracle.OracleScene(scenes.cornell_box())
    rays = osc.camera_rays(16, 16, 0)
    assert rays.tobytes() == g["rays"].tobytes()
    hits = osc.trace(rays, 0)
    assert hits.tobytes() == g["hits"].tobytes()
    assert (hits["prim"] != 0xFFFFFFFF).mean() > 0.9  # the camera looks into the box


def test_cornell_render_fixture(oracle):
    g = np.load(os.path.join(GOLDEN, "cornell_64x64_2spp.npz"))
    imgs, st = oracle.OracleScene(scenes.cornell_box()).render(64, 64, frames=2, max_depth=5, rr_depth=3)
    for k, name in enumerate(["accum", "albedo", "normal"]):
        assert imgs[k].tobytes() == g[name].tobytes(), name
    assert [st.rays_closest, st.rays_shadow] == list(g["rays"])


def test_blob_env_render_fixture(oracle):
    g = np.load(os.path.join(GOLDEN, "blob_env_64x36_2spp.npz"))
    osc = oracle.OracleScene(scenes.bunny_class(subdivisions=2), envmap=g["env"])
    imgs, st = osc.render(64, 36, frames=2, max_depth=4, rr_depth=2, env_rotation=30.0, env_intensity=1.5)
    # the scene is built with numpy transcendentals (icosphere normalisation is exact, hash noise is not libm-free):
    # compare with a tolerance so that a different numpy/libm build cannot fail the pin
    for k, name in enumerate(["accum", "albedo", "normal"]):
        d = np.abs(imgs[k] - g[name])
        assert np.mean(d.max(axis=-1) > 1e-3) < 0.02, name


def test_frame_accumulation_is_incremental(oracle):
    """rendering frames [0,2) then [2,4) into the same images == rendering [0,4) at once (running mean, RENDER_SPEC §8)"""
    osc = oracle.OracleScene(scenes.cornell_box())
    a, _ = osc.render(32, 32, frames=4)
    b, _ = osc.render(32, 32, frames=2)
    b, _ = osc.render(32, 32, frames=2, first_frame=2, images=b)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_rect_render_is_position_independent(oracle):
    """RNG is keyed by global pixel id: a sub-rectangle renders the same pixels as the full frame (basis of tile sharding)"""
    osc = oracle.OracleScene(scenes.cornell_box())
    full, _ = osc.render(48, 40, frames=2)
    part, _ = osc.render(48, 40, frames=2, rect=(16, 8, 40, 24))
    assert full[0][8:24, 16:40].tobytes() == part[0][8:24, 16:40].tobytes()
    assert np.all(part[0][:8] == 0)


def test_media_glass_render_fixture(oracle):
    """RENDER_SPEC 7.1c-f frozen: TIR-aware glass with an absorbing interior, an invisible ball of forward-scattering fog, a cut-out
    ground, quad light + env map (tests/golden/make_golden.py::media_scene)"""
    sys.path.insert(0, GOLDEN)
    from make_golden import media_scene
    g = np.load(os.path.join(GOLDEN, "media_glass_48x32_2spp.npz"))
    osc = oracle.OracleScene(media_scene(), envmap=g["env"])
    imgs, st = osc.render(48, 32, frames=2, max_depth=12, rr_depth=3, env_rotation=15.0)
    for k, name in enumerate(["accum", "albedo", "normal"]):  # tolerance: the scene generator uses libm (see the blob fixture)
        d = np.abs(imgs[k] - g[name])
        assert np.mean(d.max(axis=-1) > 1e-3) < 0.02, name
    assert abs(int(st.rays_closest) - int(g["rays"][0])) <= 0.01 * int(g["rays"][0])


def test_instanced_primitives_object_space_rule_frozen_and_consistent(oracle):
    """RENDER_SPEC 4.5 on the CPU tier: with instancing on, the four instances of the short block's mesh are intersected in object space —
    the frozen render (tests/golden/instanced_cornell_64x48_2spp.npz) pins that arithmetic against drift; the traversal of the oracle's own
    tree equals brute force ray for ray (both move the ray into the instance's object space); with instancing off (everything flattened)
    the same scene gives the same picture to rounding, not bit for bit"""
    sys.path.insert(0, GOLDEN)
    from make_golden import instanced_scene
    s = instanced_scene()
    g = np.load(os.path.join(GOLDEN, "instanced_cornell_64x48_2spp.npz"))
    oracle.set_instancing(True)
    try:
        osc = oracle.OracleScene(s)
        imgs, st = osc.render(64, 48, frames=2, max_depth=5, rr_depth=3)
        for k, name in enumerate(["accum", "albedo", "normal"]):
            assert imgs[k].tobytes() == g[name].tobytes(), name
        assert [int(st.rays_closest), int(st.rays_shadow)] == [int(g["rays"][0]), int(g["rays"][1])]
        mn, mx = osc.bounds()
        rays = np.concatenate([osc.camera_rays(96, 72, 0), random_rays(6000, mn - 50.0, mx + 50.0, 17)])
        for mode in (0, 1):
            assert osc.trace(rays, mode).tobytes() == osc.trace(rays, mode, brute=True).tobytes()
        hits = osc.trace(rays, 0)
    finally:
        oracle.set_instancing(False)
    flat = oracle.OracleScene(s)
    fimgs, _ = flat.render(64, 48, frames=2, max_depth=5, rr_depth=3)
    assert fimgs[0].tobytes() != imgs[0].tobytes() and np.abs(fimgs[0][..., :3] - imgs[0][..., :3]).mean() < 2e-3
    fhits = flat.trace(rays, 0)
    assert np.array_equal(fhits["prim"], hits["prim"]) or (fhits["prim"] != hits["prim"]).mean() < 1e-3  # the same triangles, up to grazing ties
    same = fhits["prim"] == hits["prim"]
    assert np.allclose(fhits["t"][same], hits["t"][same], rtol=2e-5, atol=1e-3)
    assert (fhits["t"][same] != hits["t"][same]).any()  # ... through other arithmetic


def furnace_scene():
    s = H.HalaScene()
    blob = scenes.blob_mesh(subdivisions=3, amplitude=0.0)  # a sphere
    blob.material_index = 0
    s.materials = [H.HalaMaterial(type=0, base_color=(1.0, 1.0, 1.0), roughness=0.0)]
    s.meshes = [H.HalaMesh([blob])]
    s.nodes = [H.HalaNode(name="sphere", mesh_index=0),
               H.HalaNode(name="cam", camera_index=0, local_transform=scenes.look_at_node_transform((0, 0, 4), (0, 0, 0)))]
    s.cameras = [H.HalaPerspectiveCamera(aspect=1.0, yfov=0.6)]
    return s


def test_furnace_sky(oracle):
    """white Lambertian sphere in a uniform environment: every pixel converges to the environment radiance"""
    osc = oracle.OracleScene(furnace_scene())
    imgs, _ = osc.render(32, 32, frames=64, max_depth=12, rr_depth=64, ground=(0.7, 0.7, 0.7, 1), sky=(0.7, 0.7, 0.7, 1))
    centre = imgs[0][8:24, 8:24, :3]
    assert abs(centre.mean() - 0.7) < 0.02  # energy lost only to the max_depth cut-off ((1)^12 -> none) and noise


def test_furnace_envmap_importance_sampling(oracle):
    """same furnace with a constant env MAP: exercises env_map_sample/pdf + MIS; must agree with the sky result"""
    env = np.full((16, 32, 4), 0.7, dtype=f32)
    osc = oracle.OracleScene(furnace_scene(), envmap=env)
    imgs, _ = osc.render(32, 32, frames=64, max_depth=12, rr_depth=64)
    assert abs(imgs[0][8:24, 8:24, :3].mean() - 0.7) < 0.02


DISNEY_VARIANTS = {
    "plastic": dict(metallic=0.0, roughness=0.5),
    "metal_aniso": dict(metallic=1.0, roughness=0.4, anisotropic=0.8, base_color=(0.9, 0.7, 0.4)),
    "clearcoat_sheen": dict(metallic=0.0, roughness=0.7, clearcoat=1.0, clearcoat_roughness=0.2, sheen=0.8, sheen_tint=0.5, specular_tint=0.6),
    # §7.1c: the refraction lobe (entering, leaving, total internal reflection); the env-map pass also connects THROUGH the surface
    "glass_rough": dict(metallic=0.0, roughness=0.4, specular_transmission=1.0, ior=1.5),
    "glass_tinted_partial": dict(metallic=0.0, roughness=0.25, specular_transmission=0.6, ior=1.33, base_color=(0.9, 0.6, 0.5)),
}


@pytest.mark.parametrize("variant", list(DISNEY_VARIANTS.keys()))
def test_disney_pdf_matches_sampling_and_conserves_energy(oracle, variant):
    """constant environment seen (a) as SKY: BSDF sampling only, (b) as a constant env MAP: NEE + BSDF with MIS.
    Both estimate the same integral; they agree only if disney_eval's pdf is the density disney_sample draws from.
    A passive material can never return more than it receives (furnace <= environment)."""
    s = furnace_scene()
    kw = dict(DISNEY_VARIANTS[variant])
    base = kw.pop("base_color", (1.0, 1.0, 1.0))
    s.materials = [H.HalaMaterial(type=1, base_color=base, **kw)]
    a = oracle.OracleScene(s).render(24, 24, frames=192, max_depth=6, rr_depth=64, ground=(0.7,) * 3 + (1,), sky=(0.7,) * 3 + (1,))[0][0]
    env = np.full((8, 16, 4), 0.7, dtype=f32)
    b = oracle.OracleScene(s, envmap=env).render(24, 24, frames=192, max_depth=6, rr_depth=64)[0][0]
    ma, mb = a[6:18, 6:18, :3].mean(), b[6:18, 6:18, :3].mean()
    assert abs(ma - mb) / mb < 0.03, (ma, mb)
    assert 0.2 < mb <= 0.7 * 1.02


def test_env_is_matches_brute_force_mean(oracle):
    """env-map IS (with a very bright sun texel) and plain BSDF sampling must converge to the same mean"""
    env = scenes.sky_sun_envmap(64, 32, sun_radius_deg=6.0, sun_gain=200.0)
    s = scenes.bunny_class(subdivisions=1)
    a = oracle.OracleScene(s, envmap=env).render(24, 16, frames=256, max_depth=2, rr_depth=8)[0][0]
    # reference estimate: same scene, but many more samples
    b = oracle.OracleScene(s, envmap=env).render(24, 16, frames=1024, max_depth=2, rr_depth=8)[0][0]
    assert abs(a[..., :3].mean() - b[..., :3].mean()) / b[..., :3].mean() < 0.05


def textured_scene(size=64, disney=True, fmt_variant=False):
    """Cornell-like room with textured (base colour + normal + metallic-roughness) blocks and an emissive-mapped wall"""
    s = scenes.cornell_box()
    if disney:
        for m in s.materials[:3] + s.materials[4:]:
            m.type = 1; m.metallic = 0.5 if m is s.materials[4] else 0.0; m.roughness = 0.6
    scenes.attach_textures(s, sets=2, size=size, seed=5)
    rng = np.random.RandomState(9)
    em = H.HalaImageData(scenes.A_FORMAT_FLOAT, 16, 8, (rng.rand(8, 16, 4) * 2).astype(f32))          # RGBA32F
    bg = H.HalaImageData(scenes.A_FORMAT_BGRA_TAG, 33, 17, (rng.rand(17, 33, 4) * 255).astype(np.uint8))  # odd size, BGRA-tag quirk
    for img in (em, bg):
        k = len(s.image_data)
        s.image_data.append(img); s.image2data_mapping[k] = k; s.texture2image_mapping[k] = k
    s.materials[1].emission = (0.4, 0.4, 0.4); s.materials[1].emission_map_index = 6
    if fmt_variant:
        s.materials[2].base_color_map_index = 7
    return s


def test_texture_mips_and_fetch_vs_independent_numpy(oracle):
    s = textured_scene(size=32)
    # a 256 x 1 sRGB ramp holding every byte code: its level 0 IS the decode table (RENDER_SPEC 7.4), read here so that the 8-bit mip rule
    # below can be emulated bit for bit whatever libm's pow() rounds to
    ramp = np.zeros((1, 256, 4), np.uint8); ramp[0, :, :3] = np.arange(256)[:, None]; ramp[..., 3] = 255
    k = len(s.image_data)
    s.image_data.append(H.HalaImageData(scenes.A_FORMAT_SRGB, 256, 1, ramp)); s.image2data_mapping[k] = k; s.texture2image_mapping[k] = k
    osc = oracle.OracleScene(s)
    lut = osc.texture_level(k, 0)[0, :, 0].copy()
    assert lut[0] == 0.0 and lut[255] == 1.0 and np.all(np.diff(lut) > 0)
    for tex in (0, 1, 6, 7):
        w, h, mips = osc.texture_info(tex)
        img = s.image_data[tex]
        assert (w, h) == (img.width, img.height)
        assert mips == int(np.ceil(np.log2(max(w, h)))) + 1  # gpu_uploader.rs:366
        # level 0 decode
        d = np.asarray(img.data)
        if img.format == scenes.A_FORMAT_FLOAT:
            l0 = d.astype(f32)
        else:
            x = d.astype(np.float64) / 255.0
            if img.format == scenes.A_FORMAT_SRGB:
                rgb = np.where(x[..., :3] <= 0.04045, x[..., :3] / 12.92, ((x[..., :3] + 0.055) / 1.055) ** 2.4)
                l0 = np.concatenate([rgb, x[..., 3:]], -1).astype(f32)
                l0[..., 3] = (d[..., 3].astype(f32) / f32(255))
            else:
                l0 = (d.astype(f32) / f32(255))
                if img.format == scenes.A_FORMAT_BGRA_TAG:
                    l0 = l0[..., [2, 1, 0, 3]]
        got0 = osc.texture_level(tex, 0)
        assert np.abs(got0 - l0).max() <= 1.2e-7  # sRGB pow(): libm vs numpy, <= 1 ulp
        # every further level is the 2x2 box filter of the previous one (edge-clamped), bit-exact
        prev = got0
        for l in range(1, mips):
            # 8-bit images stay 8-bit at every level: UNORM floor(x * 255 + 0.5), sRGB the nearest code (the number of midpoints
            # below x); the level holds what those bytes decode to (the float32 emulation lives in tests/first_hit_ref.py)
            exp = first_hit_ref.mip_level_f32(prev, w, h, l, img.format, lut)
            cur = osc.texture_level(tex, l)
            assert cur.tobytes() == exp.astype(f32).tobytes(), (tex, l)
            prev = cur
        # bilinear REPEAT fetch at level 0 against an independent float32 emulation
        rng = np.random.RandomState(tex)
        uv = (rng.rand(200, 2) * 3 - 1).astype(f32)
        got = osc.sample_texture(tex, np.concatenate([uv, np.zeros((200, 1), f32)], 1))
        for k in range(200):
            x = f32(f32(uv[k, 0] * f32(w)) - f32(0.5)); y = f32(f32(uv[k, 1] * f32(h)) - f32(0.5))
            x0, y0 = np.floor(x), np.floor(y)
            fx, fy = f32(x - x0), f32(y - y0)
            ix0, iy0 = int(x0) % w, int(y0) % h
            ix1, iy1 = (ix0 + 1) % w, (iy0 + 1) % h
            gx, gy = f32(f32(1) - fx), f32(f32(1) - fy)
            top = (got0[iy0, ix0] * gx).astype(f32) + (got0[iy0, ix1] * fx).astype(f32)
            bot = (got0[iy1, ix0] * gx).astype(f32) + (got0[iy1, ix1] * fx).astype(f32)
            exp = (top.astype(f32) * gy).astype(f32) + (bot.astype(f32) * fy).astype(f32)
            assert got[k].tobytes() == exp.astype(f32).tobytes()
    # trilinear: lod 1.5 = mean of levels 1 and 2; lod beyond the chain clamps to the last level
    q = np.array([[0.3, 0.6, 1.0], [0.3, 0.6, 2.0], [0.3, 0.6, 1.5], [0.3, 0.6, 99.0], [0.3, 0.6, -3.0], [0.3, 0.6, 0.0]], f32)
    r = osc.sample_texture(0, q)
    assert np.array_equal(r[2], (r[0] * f32(0.5) + r[1] * f32(0.5)).astype(f32))
    assert np.array_equal(r[3], osc.texture_level(0, osc.texture_info(0)[2] - 1)[0, 0]) and np.array_equal(r[4], r[5])


def test_textured_render_changes_image_and_is_deterministic(oracle):
    s = textured_scene(size=32)
    a = oracle.OracleScene(s).render(40, 40, frames=2)[0]
    b = oracle.OracleScene(s).render(40, 40, frames=2)[0]
    plain = scenes.cornell_box()
    c = oracle.OracleScene(plain).render(40, 40, frames=2)[0]
    assert a[0].tobytes() == b[0].tobytes() and not np.array_equal(a[0], c[0])
    assert np.isfinite(a[0]).all() and not np.array_equal(a[2], c[2])  # normal AOV shows the normal maps


def test_tile_assignment_is_a_balanced_partition(oracle):
    for tx, ty, world in [(60, 34, 8), (60, 34, 2), (7, 5, 4), (120, 68, 8), (3, 1, 8)]:
        owner, slot = oracle.tile_assignment(tx, ty, world)
        n = tx * ty
        counts = np.bincount(owner, minlength=world)
        assert counts.max() - counts.min() <= 1 and counts.sum() == n
        keys = owner.astype(np.int64) * (n + 1) + slot
        assert len(np.unique(keys)) == n  # (owner, slot) is unique per tile
        assert slot.max() == (n + world - 1) // world - 1


# ---- the 4-wide node format on the CPU tier ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "blob", "sheets"])
def test_bvh4_traversal_and_validation_on_the_oracles_own_tree(oracle, name):
    """RENDER_SPEC §4.1b / §4.4b without a GPU: the oracle's SAH tree converted to compressed 4-wide nodes must pass the
    structural check, and traversing it must give exactly the hits of the BVH2 traversal and of brute force"""
    s = {"cornell": lambda: scenes.cornell_box(), "blob": lambda: scenes.bunny_class(subdivisions=3),
         "sheets": lambda: scenes.stacked_sheets(count=512)}[name]()
    osc = oracle.OracleScene(s)
    nodes, tris = osc.export_bvh4()
    # (the oracle's builder boxes v0, v0 + e1, v0 + e2 — what its traversal intersects — so no exact-vertex reference here)
    rc, depth = oracle.validate_bvh(nodes, tris, None)
    assert rc == 0 and depth >= 1
    rng = np.random.RandomState(4)
    mn, mx = osc.bounds()
    pad = (mx - mn) * 0.3
    n = 4000
    rays = np.zeros(n, dtype=H._abi.RAY_DTYPE)
    rays["origin"] = rng.uniform(mn - pad, mx + pad, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["direction"] = d
    rays["tmax"] = 3.0e38
    rays = np.concatenate([rays, osc.camera_rays(40, 40, 0)])
    for mode in (0, 1):
        got, cnt = oracle.trace_on_bvh(nodes, tris, rays, mode)
        assert got.tobytes() == osc.trace(rays, mode).tobytes()
        assert got.tobytes() == osc.trace(rays, mode, brute=True).tobytes()
        assert cnt[0] >= len(rays)  # every ray visits at least the root
    # a corrupted node must be caught: shrink one child's high planes
    bad = nodes.copy()
    bad[0, 7] = 0  # qhi.x of all four children of the root
    assert oracle.validate_bvh(bad, tris, None)[0] != 0


def test_exp_neg_poly_accuracy(oracle):
    """RENDER_SPEC §7.1e: the exponential the absorbing media use — no libm, same bits on CPU and GPU by construction"""
    x = -np.concatenate([np.linspace(0, 20, 100001), np.logspace(-8, 2, 2001)]).astype(f32)
    got = oracle.probe_exp_neg(x)
    want = np.exp(x.astype(np.float64))
    ok = want > 1e-37
    assert np.max(np.abs(got[ok] - want[ok]) / want[ok]) < 4e-6
    assert oracle.probe_exp_neg(np.array([0.0, 1.0, -1e9], dtype=f32)).tolist() == [1.0, 1.0, 0.0]
    assert np.all(np.diff(got[:100001]) <= 0)  # monotone along the sweep


def test_absorbing_glass_tints_with_thickness(oracle):
    """white glass sphere with a red-absorbing medium in a white furnace: what comes through the thick centre is darker and more
    saturated than the rim, channels the medium does not absorb pass as through clear glass"""
    s = furnace_scene()
    kw = dict(type=1, base_color=(1.0, 1.0, 1.0), metallic=0.0, roughness=0.05, specular_transmission=1.0, ior=1.3)
    s.materials = [H.HalaMaterial(**kw)]
    clear = oracle.OracleScene(s).render(32, 32, frames=96, max_depth=10, rr_depth=64, ground=(0.7,) * 3 + (1,), sky=(0.7,) * 3 + (1,))[0][0]
    s.materials = [H.HalaMaterial(medium=H.HalaMedium(1, (1.0, 0.3, 0.3), 1.2, 0.0), **kw)]
    tinted = oracle.OracleScene(s).render(32, 32, frames=96, max_depth=10, rr_depth=64, ground=(0.7,) * 3 + (1,), sky=(0.7,) * 3 + (1,))[0][0]
    c, t = clear[12:20, 12:20, :3].mean(axis=(0, 1)), tinted[12:20, 12:20, :3].mean(axis=(0, 1))
    assert abs(t[0] - c[0]) < 0.03 * c[0]          # red passes untouched (sigma_r = 0)
    assert t[1] < 0.6 * c[1] and t[2] < 0.6 * c[2]  # green and blue are absorbed over ~2 radii


def test_log_poly_accuracy(oracle):
    """RENDER_SPEC §7.1f: the logarithm the free-flight sampling uses — no libm, same bits on CPU and GPU by construction"""
    x = np.concatenate([np.linspace(2.0 ** -24, 1.0, 200001), np.logspace(-7.2, 0, 4001), np.logspace(0, 6, 1001)]).astype(f32)
    got = oracle.probe_log(x).astype(np.float64)
    want = np.log(x.astype(np.float64))
    assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-6)) < 4e-7 or np.max(np.abs(got - want)) < 2e-7
    assert np.max(np.abs(got - want)) < 2e-6  # absolute, over |ln x| <= 17
    assert oracle.probe_log(np.array([1.0], dtype=f32))[0] == 0.0
    k = np.arange(1, 2 ** 12, dtype=np.float64) * 2.0 ** -24  # the smallest arguments 1 - xi can take
    assert np.all(np.isfinite(oracle.probe_log(k.astype(f32))))


def test_hg_sample_statistics(oracle):
    """unit vectors, mean cosine = g (the defining property of Henyey-Greenstein), isotropic at g = 0"""
    rng = np.random.RandomState(3)
    u1, u2 = rng.rand(200000).astype(f32), rng.rand(200000).astype(f32)
    d = np.array([0.3, -0.5, 0.81], dtype=f32); d /= np.linalg.norm(d)
    for g in (0.0, 0.6, -0.4, 0.95):
        w = oracle.probe_hg(d, g, u1, u2).astype(np.float64)
        assert np.max(np.abs(np.linalg.norm(w, axis=1) - 1.0)) < 1e-5
        assert abs((w @ d.astype(np.float64)).mean() - g) < 5e-3


def scatter_scene(density, colour=(1.0, 1.0, 1.0), g=0.0):
    """a ball of scattering medium behind an invisible boundary (opacity 0, 7.1d: always passed straight through; the medium of
    7.1e/f acts before the opacity test): a bare participating medium"""
    s = furnace_scene()
    s.materials = [H.HalaMaterial(type=0, base_color=(1.0, 1.0, 1.0), roughness=0.5, opacity=0.0, medium=H.HalaMedium(2, colour, density, g))]
    return s


FURNACE = dict(frames=64, max_depth=64, rr_depth=255, ground=(0.7,) * 3 + (1,), sky=(0.7,) * 3 + (1,))


def test_scattering_medium_white_furnace(oracle):
    """7.1f: a non-absorbing scattering medium only redirects light: in a uniform environment every pixel still sees the environment
    radiance - thin and thick media, isotropic and forward-peaked phase functions; what is lost is the max_depth cut-off"""
    for density, g in ((0.5, 0.0), (2.0, 0.0), (2.0, 0.7), (3.0, -0.3)):
        img = oracle.OracleScene(scatter_scene(density, g=g)).render(32, 32, **FURNACE)[0][0]
        assert abs(img[10:22, 10:22, :3].mean() - 0.7) < 0.01, (density, g, img[10:22, 10:22, :3].mean())


def test_scattering_medium_albedo_darkens(oracle):
    """single-scattering albedo < 1 in one channel: that channel loses energy at every scattering event, the others do not;
    a denser ball scatters more often and gets darker in that channel"""
    c1 = oracle.OracleScene(scatter_scene(1.0, colour=(1.0, 0.5, 1.0))).render(32, 32, **FURNACE)[0][0][10:22, 10:22, :3].mean(axis=(0, 1))
    c3 = oracle.OracleScene(scatter_scene(3.0, colour=(1.0, 0.5, 1.0))).render(32, 32, **FURNACE)[0][0][10:22, 10:22, :3].mean(axis=(0, 1))
    for c in (c1, c3):
        assert abs(c[0] - 0.7) < 0.01 and abs(c[2] - 0.7) < 0.01
    assert c3[1] < c1[1] < 0.62


def test_scattering_medium_blurs_the_horizon(oracle):
    """a dense ball in front of a black ground / white sky: the pixels through the ball see a mix instead of the sharp horizon"""
    img = oracle.OracleScene(scatter_scene(6.0)).render(32, 32, frames=64, max_depth=64, rr_depth=255, ground=(0, 0, 0, 1), sky=(1, 1, 1, 1))[0][0]
    centre = img[12:20, 12:20, 0]
    assert 0.1 < centre.mean() < 0.9 and centre.std() < 0.3


def test_glass_is_energy_conserving_from_inside(oracle):
    """§7.1c: the transmissive share of the specular lobe reflects by the exact dielectric Fresnel term, so light that reaches a glass
    boundary from inside beyond the critical angle is totally reflected instead of lost: a glass ball stays a white furnace even
    when a scattering interior sends light at the boundary from every direction (a Schlick-weighted lobe gave 0.63 / 0.47 here)"""
    for density in (0.0, 0.5, 3.0):
        s = furnace_scene()
        kw = dict(type=1, base_color=(1.0, 1.0, 1.0), metallic=0.0, roughness=0.05, specular_transmission=1.0, ior=1.3)
        s.materials = [H.HalaMaterial(medium=H.HalaMedium(2, (1.0, 1.0, 1.0), density, 0.0), **kw)]
        img = oracle.OracleScene(s).render(32, 32, **FURNACE)[0][0]
        assert abs(img[10:22, 10:22, :3].mean() - 0.7) < 0.01, density


def fog_over_floor_scene(with_fog=True):
    """a quad light above a floor, an invisible (opacity 0) ball of fog between them"""
    s = H.HalaScene()
    floor = scenes._merge_quads([((-3, 0, 3), (3, 0, 3), (3, 0, -3), (-3, 0, -3))])
    floor.material_index = 0
    ball = scenes.blob_mesh(subdivisions=2, amplitude=0.0)
    ball.material_index = 1
    s.materials = [H.HalaMaterial(type=0, base_color=(0.8, 0.8, 0.8), roughness=0.5),
                   H.HalaMaterial(type=0, base_color=(1.0, 1.0, 1.0), roughness=0.5, opacity=0.0, medium=H.HalaMedium(2, (1.0, 1.0, 1.0), 0.3, 0.0))]
    s.meshes = [H.HalaMesh([floor])] + ([H.HalaMesh([ball])] if with_fog else [])
    m = np.eye(4, dtype=f32); m[:3, 3] = (0.0, 1.5, 0.0)
    s.nodes = [H.HalaNode(name="floor", mesh_index=0)]
    if with_fog:
        s.nodes.append(H.HalaNode(name="fog", mesh_index=1, local_transform=m))
    lm = np.eye(4, dtype=f32); lm[:3, :3] = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=f32); lm[:3, 3] = (0.0, 4.0, 0.0)  # cross(X, Y) of the node points down
    s.nodes.append(H.HalaNode(name="light", light_index=0, local_transform=lm))
    s.lights = [H.HalaLight(color=(1.0, 1.0, 1.0), intensity=20.0, light_type=3, params=(1.0, 1.0))]
    s.nodes.append(H.HalaNode(name="cam", camera_index=0, local_transform=scenes.look_at_node_transform((0, 5, 6), (0, 0, 0))))
    s.cameras = [H.HalaPerspectiveCamera(aspect=1.0, yfov=0.6)]
    return s


def test_invisible_surfaces_do_not_block_shadow_rays(oracle):
    """§7.1d: the opacity-0 boundary of a thin fog ball between a light and a floor casts no shadow — the floor under it is as bright
    as without the ball (thin medium: few paths scatter), and any-hit rays agree between the BVH and brute force"""
    kw = dict(frames=32, max_depth=6, rr_depth=64, ground=(0, 0, 0, 1), sky=(0, 0, 0, 1))
    fog = oracle.OracleScene(fog_over_floor_scene(True))
    lit = fog.render(32, 32, **kw)[0][0][12:20, 12:20, :3].mean()
    ref = oracle.OracleScene(fog_over_floor_scene(False)).render(32, 32, **kw)[0][0][12:20, 12:20, :3].mean()
    # the boundary itself casts no shadow; the fog behind it does attenuate the connections that cross it (7.1g: density 0.3 over at most
    # 2 units: transmittance >= 0.55) and scatters some light back in
    assert ref > 0.05 and 0.5 * ref < lit < 0.98 * ref
    rays = random_rays(4000, np.array((-3, 0.05, -3.0)), np.array((3, 4, 3.0)), 11)
    assert fog.trace(rays, 1).tobytes() == fog.trace(rays, 1, brute=True).tobytes()
    down = rays.copy(); down["origin"] = (0.0, 3.9, 0.0); down["direction"] = (0.0, -1.0, 0.0); down["tmin"] = 0.0; down["tmax"] = 3.8
    assert (fog.trace(down[:4], 1)["t"] < 0).all()       # straight through the ball: unoccluded for a shadow ray ...
    assert (fog.trace(down[:4], 0)["prim"] != 0xFFFFFFFF).all()  # ... while a closest-hit ray finds the boundary


def sheet_over_floor_scene(opacity=1.0, alpha_checker=False, sheets=1):
    """a quad light above a floor with `sheets` large horizontal sheets between them: material opacity `opacity`, optionally a
    base-colour map whose alpha is a 16x16 checker of 0 / 1 (a cut-out); the camera sits below the sheets and looks at the floor"""
    s = H.HalaScene()
    floor = scenes._merge_quads([((-6, 0, 6), (6, 0, 6), (6, 0, -6), (-6, 0, -6))])
    floor.material_index = 0
    quads = [((-6, 2.0 + 0.2 * k, -6), (6, 2.0 + 0.2 * k, -6), (6, 2.0 + 0.2 * k, 6), (-6, 2.0 + 0.2 * k, 6)) for k in range(sheets)]
    sheet = scenes._merge_quads(quads)
    sheet.material_index = 1
    s.materials = [H.HalaMaterial(type=0, base_color=(0.8, 0.8, 0.8), roughness=0.5),
                   H.HalaMaterial(type=0, base_color=(1.0, 1.0, 1.0), roughness=0.5, opacity=opacity)]
    if alpha_checker:
        n = 64
        yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        px = np.full((n, n, 4), 255, dtype=np.uint8)
        px[..., 3] = np.where(((yy // 4) + (xx // 4)) % 2 == 0, 255, 0)
        s.image_data = [H.HalaImageData(1, n, n, px)]  # HALA_FORMAT_R8G8B8A8_SRGB
        s.image2data_mapping = {0: 0}; s.texture2image_mapping = {0: 0}
        s.materials[1].base_color_map_index = 0
    s.meshes = [H.HalaMesh([floor]), H.HalaMesh([sheet])]
    s.nodes = [H.HalaNode(name="floor", mesh_index=0), H.HalaNode(name="sheet", mesh_index=1)]
    lm = np.eye(4, dtype=f32); lm[:3, :3] = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=f32); lm[:3, 3] = (0.0, 4.0, 0.0)
    s.nodes.append(H.HalaNode(name="light", light_index=0, local_transform=lm))
    s.lights = [H.HalaLight(color=(1.0, 1.0, 1.0), intensity=20.0, light_type=3, params=(1.0, 1.0))]
    s.nodes.append(H.HalaNode(name="cam", camera_index=0, local_transform=scenes.look_at_node_transform((0, 1.5, 2.5), (0, 0, 0))))
    s.cameras = [H.HalaPerspectiveCamera(aspect=1.0, yfov=0.5)]
    return s


def test_translucent_surfaces_shadow_in_proportion(oracle):
    """§7.1d, connections: a sheet of opacity a between light and floor lets a connection through with probability 1 - a (decided per
    (connection key, triangle): independent of the traversal), so the directly lit floor is (1 - a) times as bright; two sheets
    multiply; a base-colour map whose alpha is a half-covered 0 / 1 checker acts like opacity 1/2; opacity 1 is black, 0 unshadowed.
    max_depth 1: direct light only; the camera sits below the sheets."""
    kw = dict(frames=48, max_depth=1, rr_depth=64, ground=(0, 0, 0, 1), sky=(0, 0, 0, 1))

    def lit(**scene_kw):
        return float(oracle.OracleScene(sheet_over_floor_scene(**scene_kw)).render(32, 32, **kw)[0][0][8:24, 8:24, :3].mean())

    ref = lit(opacity=0.0)
    assert ref > 0.05
    assert lit(opacity=1.0) == 0.0
    for a in (0.25, 0.5, 0.8):
        assert abs(lit(opacity=a) / ref - (1.0 - a)) < 0.04, a
    assert abs(lit(opacity=0.5, sheets=2) / ref - 0.25) < 0.03
    assert abs(lit(opacity=1.0, alpha_checker=True) / ref - 0.5) < 0.05
    assert abs(lit(opacity=0.5, alpha_checker=True) / ref - 0.75) < 0.05


def test_translucent_any_hit_is_traversal_independent(oracle):
    """the blocking decision is a function of (ray key, triangle, alpha at the hit) only: the BVH traversal, whatever order it visits
    the sheets in, agrees with brute force over all triangles, ray for ray"""
    s = sheet_over_floor_scene(opacity=0.6, alpha_checker=True, sheets=5)
    osc = oracle.OracleScene(s)
    rays = random_rays(6000, np.array((-5, 0.05, -5.0)), np.array((5, 4, 5.0)), 5)
    a, b = osc.trace(rays, 1), osc.trace(rays, 1, brute=True)
    assert a.tobytes() == b.tobytes()
    occluded = float((a["t"] > 0).mean())
    solid = oracle.OracleScene(sheet_over_floor_scene(opacity=1.0, sheets=5)).trace(rays, 1)
    assert 0.1 < occluded < float((solid["t"] > 0).mean())  # some connections get through five 0.3-opaque sheets


def box_mesh(lo, hi):
    """closed axis-aligned box, 12 triangles, geometric normals (cross(e1, e2)) pointing outward"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    quads = [((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)),  # -x
             ((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)),  # +x
             ((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)),  # -y
             ((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)),  # +y
             ((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)),  # -z
             ((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1))]  # +z
    m = scenes._merge_quads(quads)
    p = m.vertices["position"].reshape(-1, 4, 3)
    for q, quad in zip(p, quads):  # _quad's normal is (p1 - p0) x (p3 - p0): check it points away from the box centre
        n = np.cross(q[1] - q[0], q[3] - q[0])
        assert np.dot(n, q[0] - (np.array(lo) + np.array(hi)) / 2) > 0
    return m


def slab_over_floor_scene(medium, slab=True, opacity=0.0):
    """a small quad light high above a floor, a wide closed slab (y in [2, 2.5]) of `medium` behind an invisible boundary between them;
    the camera sits below the slab and looks at the floor under the light"""
    s = H.HalaScene()
    floor = scenes._merge_quads([((-6, 0, 6), (6, 0, 6), (6, 0, -6), (-6, 0, -6))])
    floor.material_index = 0
    s.materials = [H.HalaMaterial(type=0, base_color=(0.8, 0.8, 0.8), roughness=0.5),
                   H.HalaMaterial(type=0, base_color=(1.0, 1.0, 1.0), roughness=0.5, opacity=opacity, medium=medium)]
    s.meshes = [H.HalaMesh([floor])]
    s.nodes = [H.HalaNode(name="floor", mesh_index=0)]
    if slab:
        box = box_mesh((-6, 2.0, -6), (6, 2.5, 6))
        box.material_index = 1
        s.meshes.append(H.HalaMesh([box]))
        s.nodes.append(H.HalaNode(name="slab", mesh_index=1))
    lm = np.eye(4, dtype=f32); lm[:3, :3] = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=f32); lm[:3, 3] = (0.0, 8.0, 0.0)
    s.nodes.append(H.HalaNode(name="light", light_index=0, local_transform=lm))
    s.lights = [H.HalaLight(color=(1.0, 1.0, 1.0), intensity=400.0, light_type=3, params=(0.2, 0.2))]
    s.nodes.append(H.HalaNode(name="cam", camera_index=0, local_transform=scenes.look_at_node_transform((0, 1.5, 1.0), (0, 0, 0))))
    s.cameras = [H.HalaPerspectiveCamera(aspect=1.0, yfov=0.25)]
    return s


def test_media_attenuate_connections_beer_lambert(oracle):
    """§7.1g: a connection that crosses a medium behind an invisible boundary keeps exp(-sigma x length) of its contribution, per channel:
    ABSORB sigma = density x (1 - colour), SCATTER sigma = density.  Slab of thickness 0.5 between a small light 8 above the floor and the
    floor under it (connections nearly vertical: length 0.5 / cos, cos > 0.99 in the measured patch); max_depth 1: direct light only."""
    kw = dict(frames=16, max_depth=1, rr_depth=64, ground=(0, 0, 0, 1), sky=(0, 0, 0, 1))

    def lit(**scene_kw):
        return oracle.OracleScene(slab_over_floor_scene(**scene_kw)).render(32, 32, **kw)[0][0][8:24, 8:24, :3].reshape(-1, 3).mean(axis=0)

    ref = lit(medium=H.HalaMedium(), slab=False)
    assert ref.min() > 0.05
    a = lit(medium=H.HalaMedium(1, (0.2, 0.5, 0.8), 2.0, 0.0))  # sigma = (1.6, 1.0, 0.4) -> tau = (0.8, 0.5, 0.2)
    assert np.allclose(a / ref, np.exp(-np.array([0.8, 0.5, 0.2])), rtol=0.02), a / ref
    b = lit(medium=H.HalaMedium(2, (0.9, 0.9, 0.9), 1.5, 0.0))  # extinction 1.5 in every channel -> tau = 0.75 (direct light only)
    assert np.allclose(b / ref, np.exp(-0.75), rtol=0.02), b / ref
    c = lit(medium=H.HalaMedium(3, (0.5, 0.5, 0.5), 2.0, 0.0))  # EMISSIVE: connections pass unattenuated
    assert np.allclose(c / ref, 1.0, rtol=1e-6)
    # an opaque boundary blocks the connection whatever is inside; half-opaque: half of the connections, each attenuated
    assert lit(medium=H.HalaMedium(1, (0.2, 0.5, 0.8), 2.0, 0.0), opacity=1.0).max() == 0.0
    # two faces of opacity 0.5 -> a quarter of the connections get through both
    d = lit(medium=H.HalaMedium(1, (0.2, 0.5, 0.8), 2.0, 0.0), opacity=0.5)
    assert np.allclose(d / ref, 0.25 * np.exp(-np.array([0.8, 0.5, 0.2])), rtol=0.25)
    # traversal independence with media in the way: BVH == brute force for occlusion
    osc = oracle.OracleScene(slab_over_floor_scene(medium=H.HalaMedium(1, (0.2, 0.5, 0.8), 2.0, 0.0), opacity=0.5))
    rays = random_rays(3000, np.array((-5, 0.05, -5.0)), np.array((5, 4, 5.0)), 21)
    assert osc.trace(rays, 1).tobytes() == osc.trace(rays, 1, brute=True).tobytes()


def test_scattering_medium_white_furnace_with_next_event_estimation(oracle):
    """§7.1f + §7.1g: the same furnace under a constant environment MAP: every scattering vertex now connects to the environment with the
    phase function as its BSDF (value = pdf), the connection is attenuated by the medium it still has to cross, and the phase-sampled
    direction carries its pdf to the next vertex's MIS weight — the estimator stays unbiased (radiance = environment) for thin / thick,
    isotropic / forward / backward media, also inside glass (no connection gets out: only the MIS weights change)"""
    env = np.full((16, 32, 4), 0.7, dtype=f32)
    kw = dict(frames=64, max_depth=64, rr_depth=255)
    for density, g in ((0.5, 0.0), (2.0, 0.0), (2.0, 0.7), (3.0, -0.3)):
        img = oracle.OracleScene(scatter_scene(density, g=g), envmap=env).render(32, 32, **kw)[0][0]
        assert abs(img[10:22, 10:22, :3].mean() - 0.7) < 0.01, (density, g, img[10:22, 10:22, :3].mean())
    s = furnace_scene()
    s.materials = [H.HalaMaterial(type=1, base_color=(1.0, 1.0, 1.0), metallic=0.0, roughness=0.05, specular_transmission=1.0, ior=1.3,
                                  medium=H.HalaMedium(2, (1.0, 1.0, 1.0), 2.0, 0.3))]
    img = oracle.OracleScene(s, envmap=env).render(32, 32, **kw)[0][0]
    assert abs(img[10:22, 10:22, :3].mean() - 0.7) < 0.01


def test_scattering_vertices_see_the_light_directly(oracle):
    """a fog ball under a small quad light in a black world: with next-event estimation at the scattering vertices the in-scattered light
    shows after a handful of samples (before, a path had to hit the 1x1 light by chance); 8 spp agree with 256 spp within the noise"""
    kw = dict(max_depth=8, rr_depth=64, ground=(0, 0, 0, 1), sky=(0, 0, 0, 1))
    s = fog_over_floor_scene(True)
    s.materials[1].medium = H.HalaMedium(2, (1.0, 1.0, 1.0), 1.5, 0.0)
    osc = oracle.OracleScene(s)
    few = osc.render(32, 32, frames=8, **kw)[0][0]
    many = osc.render(32, 32, frames=256, **kw)[0][0]
    ball = (slice(6, 16), slice(11, 21))  # pixels that see the fog ball
    a, b = float(few[ball][..., :3].mean()), float(many[ball][..., :3].mean())
    assert b > 0.02 and abs(a - b) < 0.15 * b


def test_half_transparent_sphere_stays_a_furnace_under_an_env_map(oracle):
    """§6 / §7.1d: a camera path that skips surfaces (opacity < 1) before it reaches the environment MAP has no sampled direction behind it:
    the environment counts in full (prev_pdf starts at 1e18: power(1e18, b) = 1).  A white sphere of opacity 0.5 in a constant
    environment — half of the paths pass straight through it, twice — converges to the environment radiance like the opaque one."""
    env = np.full((16, 32, 4), 0.7, dtype=f32)
    s = furnace_scene()
    s.materials[0].opacity = 0.5
    img = oracle.OracleScene(s, envmap=env).render(32, 32, frames=64, max_depth=16, rr_depth=64)[0][0]
    assert abs(img[8:24, 8:24, :3].mean() - 0.7) < 0.02
    assert abs(img[0:3, 0:3, :3].mean() - 0.7) < 1e-6  # pixels that miss the sphere
