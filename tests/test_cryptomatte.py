"""Cryptomatte ID mattes (docs/RENDER_SPEC.md 15): per pixel, view and layer, a ranked id -> coverage table over every sample.
CPU tier: MurmurHash3 known answers of the library and of the numpy twin (tests/cryptomatte_ref.py), the exponent flip, hand-written fold
cases of the twin, the OpenEXR writer against a small reader kept here (zlib, predictor and interleave undone), the header, and the
descriptor's refusals before any device call.  GPU tier: records and ranked floats against the twin on the oracle's first hits, bit for
bit — random scenes, update_batch, two-level trees, views, adaptive sampling, pass fusion and the tail overlap, a refit after a scene
edit, a frame of many small objects (other > 0) — images 0-5 and the statistics unchanged by the feature, the EXR and the matte of a
name, the manifests, and the refusals."""
import ctypes as C
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest

import cryptomatte_ref as R
from conftest import ROOT
from hala_renderer_amd import scenes

gpu = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
W, H = 61, 37
SEEDS = [17, 25, 20, 12, 22]  # the random scenes of test_aovs.py: every light type, opacity, media, thin lens, orthographic, env map
ENTRY_POINTS = ("hala_rt_set_cryptomatte", "hala_rt_read_cryptomatte", "hala_rt_read_cryptomatte_records", "hala_rt_get_cryptomatte_manifest",
                "hala_rt_save_cryptomatte")
KNOWN = [(b"", 0, 0x00000000), (b"hello", 0, 0x248BFA47), (b"\0\0\0\0", 0, 0x2362F9DE), (b"", 1, 0x514E28B7), (b"", 0xFFFFFFFF, 0x81F16F39),
         (b"aaaa", 0x9747B28C, 0x5A97808A), (b"Hello, world!", 0x9747B28C, 0x24884CBA),
         (b"The quick brown fox jumps over the lazy dog", 0x9747B28C, 0x2FA826CD)]


def lib_hash(halart, name: bytes):
    raw, idv = C.c_uint32(), C.c_uint32()
    halart.check(halart.load_library().hala_cryptomatte_hash(name, C.byref(raw), C.byref(idv)))
    return raw.value, idv.value


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data,seed,want", KNOWN)
def test_twin_murmur3_known_answers(data, seed, want):
    assert R.murmur3_32(data, seed) == want


def test_library_hash_known_answers_and_twin(halart):
    # the C entry point takes a C string: seed 0 only, no 0 byte inside
    for data, seed, want in KNOWN:
        if seed == 0 and b"\0" not in data:
            assert lib_hash(halart, data)[0] == want, data
    rs = np.random.RandomState(1)
    for n in range(200):
        name = "".join(chr(int(c)) for c in rs.randint(1, 0x3000, size=n % 23)).encode("utf-8")
        raw, idv = lib_hash(halart, name)
        assert raw == R.murmur3_32(name) and idv == R.crypto_id(raw), name


def test_exponent_flip(halart):
    found = {}
    for i in range(200000):
        name = f"obj{i}"
        e = (R.murmur3_32(name.encode()) >> 23) & 0xFF
        if e in (0, 255) and e not in found:
            found[e] = name
        if len(found) == 2:
            break
    assert set(found) == {0, 255}
    for e, name in found.items():
        raw, idv = lib_hash(halart, name.encode())
        assert (raw >> 23) & 0xFF == e and idv == raw ^ (1 << 23) == R.name_id(name)
        v = np.array([idv], u32).view(f32)[0]
        assert np.isfinite(v) and abs(v) >= np.finfo(f32).tiny
    raw, idv = lib_hash(halart, b"hello")
    assert idv == raw  # exponent neither 0 nor 255: unchanged


def record(n, other, *pairs):
    r = np.zeros(16, u32)
    r[0], r[1] = n, other
    for j, (i, c) in enumerate(pairs):
        r[2 + 2 * j], r[3 + 2 * j] = i, c
    return r


def test_fold_rules_of_the_twin():
    r = R.empty((1,))

    def step(has, key):
        nonlocal r
        r = R.fold(r, np.array([has]), np.array([key], u32))
        return r[0]

    assert np.array_equal(step(True, 50), record(1, 0, (50, 1)))
    assert np.array_equal(step(True, 20), record(2, 0, (20, 1), (50, 1)))  # a tie: id ascending
    assert np.array_equal(step(False, 0), record(3, 0, (20, 1), (50, 1)))  # a miss counts in n only
    assert np.array_equal(step(True, 50), record(4, 0, (50, 2), (20, 1)))  # moves up
    assert np.array_equal(step(True, 20), record(5, 0, (20, 2), (50, 2)))  # tie again
    for k in (30, 10, 40, 60, 70):
        step(True, k)
    assert np.array_equal(r[0], record(10, 0, (20, 2), (50, 2), (10, 1), (30, 1), (40, 1), (60, 1), (70, 1)))  # insertion order
    assert np.array_equal(step(True, 80), record(11, 1, (20, 2), (50, 2), (10, 1), (30, 1), (40, 1), (60, 1), (70, 1)))  # full: other
    step(True, 70)
    assert np.array_equal(step(True, 70), record(13, 1, (70, 3), (20, 2), (50, 2), (10, 1), (30, 1), (40, 1), (60, 1)))
    ids, cov = R.rank(r)
    assert ids[0].view(u32).tolist() == [70, 20, 50, 10, 30, 40] and cov[0][0] == f32(3) / f32(13)
    ids, cov = R.rank(R.empty((1,)) + np.array(record(2, 0, (9, 1)), u32))
    assert ids[0].view(u32).tolist() == [9, 0, 0, 0, 0, 0] and cov[0].tolist() == [0.5, 0, 0, 0, 0, 0]


def read_exr(path):
    """-> (channel names in file order, {attribute: (type, bytes)}, {channel: [H, W] float32}) of a single-part scanline FLOAT file"""
    d = open(path, "rb").read()
    magic, version = struct.unpack_from("<II", d, 0)
    assert magic == 20000630 and version & 0xFF == 2 and not version & 0x1A00
    p, attrs = 8, {}
    while d[p] != 0:
        e = d.index(b"\0", p); name = d[p:e].decode(); p = e + 1
        e = d.index(b"\0", p); typ = d[p:e].decode(); p = e + 1
        size, = struct.unpack_from("<I", d, p); p += 4
        attrs[name] = (typ, d[p:p + size]); p += size
    p += 1
    q, i, chans = attrs["channels"][1], 0, []
    while q[i] != 0:
        e = q.index(b"\0", i); nm = q[i:e].decode(); i = e + 1
        pt, = struct.unpack_from("<i", q, i); i += 16
        assert pt == 2
        chans.append(nm)
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    assert attrs["compression"][1] == b"\x03"
    nchunks = (h + 15) // 16
    offsets = struct.unpack_from(f"<{nchunks}Q", d, p)
    assert offsets[0] == p + 8 * nchunks
    planes = {nm: np.zeros((h, w), f32) for nm in chans}
    end = offsets[0]
    for k, off in enumerate(offsets):
        assert off == end
        y, size = struct.unpack_from("<iI", d, off)
        assert y == y0 + 16 * k
        data = d[off + 8:off + 8 + size]
        end = off + 8 + size
        lines = min(16, h - 16 * k)
        want = lines * w * 4 * len(chans)
        if size < want:
            t = np.frombuffer(zlib.decompress(data), np.uint8).astype(np.int64)
            assert t.size == want
            t = ((np.cumsum(t - 128) + 128) % 256).astype(np.uint8)  # undo the predictor
            raw = np.empty(want, np.uint8)
            half = (want + 1) // 2
            raw[0::2], raw[1::2] = t[:half], t[half:]  # undo the interleave
        else:
            raw = np.frombuffer(data, np.uint8)
        px = raw.view("<f4").reshape(lines, len(chans), w)
        for c, nm in enumerate(chans):
            planes[nm][16 * k:16 * k + lines] = px[:, c]
    assert end == len(d)
    return chans, attrs, planes


def write_exr(halart, path, planes, attrs):
    names = list(planes)
    arrs = [np.ascontiguousarray(planes[n], f32) for n in names]
    h, w = arrs[0].shape
    cn = (C.c_char_p * len(names))(*[n.encode("utf-8") for n in names])
    pp = (C.POINTER(C.c_float) * len(names))(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrs])
    an = (C.c_char_p * max(len(attrs), 1))(*[k.encode("utf-8") for k in attrs])
    av = (C.c_char_p * max(len(attrs), 1))(*[v.encode("utf-8") for v in attrs.values()])
    return halart.load_library().hala_write_exr(os.fsencode(path), w, h, len(names), cn, pp, len(attrs), an, av)


def test_exr_writer_round_trip(halart, tmp_path):
    rs = np.random.RandomState(3)
    w, h = 23, 37  # three blocks, the last one of 5 lines
    bits = rs.randint(0, 2 ** 32, size=(h, w), dtype=np.uint64).astype(u32)
    bits[0, :4] = [0x7FC00001, 0xFF800000, 0x00000001, 0x80000000]  # a NaN payload, -inf, a denormal, -0
    planes = {"Z": rs.standard_normal((h, w)).astype(f32), "B": np.zeros((h, w), f32), "A": bits.view(f32),
              "CryptoObject00.R": np.tile(np.arange(w, dtype=f32), (h, 1)), "G": rs.uniform(0, 1, (h, w)).astype(f32), "R": np.ones((h, w), f32)}
    manifest = json.dumps({'quo"te': "00000001", "back\\slash": "7f000000", "café ☃": "12345678", "new\nline": "00800000"},
                          ensure_ascii=False)
    attrs = {"cryptomatte/1234567/manifest": manifest, "cryptomatte/1234567/name": "CryptoObject", "note": "ünïcødé"}
    path = tmp_path / "t.exr"
    assert write_exr(halart, path, planes, attrs) == 0, halart.last_error()
    chans, got_attrs, got = read_exr(path)
    assert chans == sorted(planes, key=lambda s: s.encode())
    for n, p in planes.items():
        assert got[n].view(u32).tobytes() == p.view(u32).tobytes(), n
    for k, v in attrs.items():
        assert got_attrs[k] == ("string", v.encode("utf-8")), k
    assert json.loads(got_attrs["cryptomatte/1234567/manifest"][1].decode("utf-8")) == json.loads(manifest)
    for req in ("channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio", "screenWindowCenter", "screenWindowWidth"):
        assert req in got_attrs, req
    # the library's own reader (set_envmap_file) takes R, G, B, A back
    lib = halart.load_library()
    wd, ht, ch = C.c_uint32(), C.c_uint32(), C.c_uint32()
    buf = np.zeros(w * h * 4, f32)
    halart.check(lib.hala_load_float_image(os.fsencode(path), C.byref(wd), C.byref(ht), C.byref(ch), buf.ctypes.data_as(C.POINTER(C.c_float)),
                                           C.c_size_t(buf.size)))
    assert (wd.value, ht.value, ch.value) == (w, h, 4)
    want = np.stack([planes["R"], planes["G"], planes["B"], planes["A"]], -1)
    assert buf.view(u32).tobytes() == want.view(u32).tobytes()
    # refusals
    assert write_exr(halart, tmp_path / "x.exr", {"R": planes["R"], "": planes["G"]}, {}) != 0
    assert write_exr(halart, tmp_path / "x.exr", {"R": planes["R"]}, {"channels": "x"}) != 0 and "required" in halart.last_error()
    one = np.zeros(4, f32)
    cn = (C.c_char_p * 32)(*[f"c{k:02d}".encode() for k in range(32)])
    pp = (C.POINTER(C.c_float) * 32)(*[one.ctypes.data_as(C.POINTER(C.c_float))] * 32)
    assert lib.hala_write_exr(os.fsencode(tmp_path / "x.exr"), 1 << 20, 1, 32, cn, pp, 0, None, None) != 0  # a block of 2^31 bytes
    assert "2^31" in halart.last_error()


def test_header_declares_the_cryptomatte_entry_points(halart):
    text = open(os.path.join(ROOT, "include", "halart.h")).read()
    assert re.search(r"typedef struct hala_cryptomatte_desc \{.*?\} hala_cryptomatte_desc;", text, flags=re.S)
    for fn in ENTRY_POINTS:
        assert re.search(r"int " + fn + r"\(hala_rt_renderer\* r,", text), fn
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct hala_cryptomatte_desc", text, flags=re.S)
    assert m
    for w in ("RENDER_SPEC.md 15", "MurmurHash3_x86_32", "world > 1", "restarts the accumulation", "Not built"):
        assert w in m.group(1), w
    lib = C.CDLL(halart.LIB_PATH)
    for fn in ENTRY_POINTS + ("hala_cryptomatte_hash", "hala_write_exr"):
        assert fn in halart._abi.EXPORTS and hasattr(lib, fn), fn
    assert C.sizeof(halart._abi.CryptomatteDesc) == 24


def descriptor(halart, mask=7, names=None, null_names=False, reserved=(0, 0)):
    names = [n.encode() for n in (names or ["a", "b"])]
    arr = (C.c_char_p * len(names))(*names)
    d = halart._abi.CryptomatteDesc(layer_mask=mask, material_name_count=len(names), material_names=None if null_names else C.cast(arr, C.POINTER(C.c_char_p)))
    d.reserved[0], d.reserved[1] = reserved
    return d, arr


@pytest.mark.parametrize("kw,word", [(dict(mask=0), "layer_mask"), (dict(mask=8), "layer_mask"), (dict(null_names=True), "null"),
                                     (dict(reserved=(0, 1)), "reserved")])
def test_invalid_descriptors_are_refused_before_any_device_call(halart, kw, word):
    d, keep = descriptor(halart, **kw)
    assert halart.load_library().hala_rt_set_cryptomatte(None, C.byref(d)) == 1  # before the renderer handle is looked at
    assert word in halart.last_error()
    d, keep = descriptor(halart)
    assert halart.load_library().hala_rt_set_cryptomatte(None, C.byref(d)) == 1 and "null" in halart.last_error()


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------
def make(halart, scene, kw, env=None, layers=R.LAYERS, aovs=None, build=None, names=None):
    r = halart.HalaRenderer("crypto", kw["width"], kw["height"], kw["max_depth"], kw["rr_depth"], *kw["tonemap"], 0)
    if build is not None:
        r.set_build_options(**build)
    if env is not None:
        r.set_envmap(env, kw["env_rotation"])
    r.set_env_intensity(kw.get("env_intensity", 1.0))
    r.set_exposure_value(kw.get("exposure", 1.0))
    r.set_scene(scene)
    r.commit()
    if aovs is not None:
        r.set_aovs(*aovs)
    if layers is not None:
        r.set_cryptomatte(layers, material_names=names)
    return r


def kw_of(w=W, h=H, md=5, rr=3, tm=(False, False, False)):
    return dict(width=w, height=h, max_depth=md, rr_depth=rr, tonemap=tm, env_rotation=0.0, env_intensity=1.0, exposure=1.0)


def assert_same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.any(got.reshape(got.shape[0], got.shape[1], -1) != want.reshape(want.shape[0], want.shape[1], -1), axis=-1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ")


def check(r, want, what, layers=R.LAYERS, view=0):
    for layer in layers:
        assert_same(r.read_cryptomatte_records(layer, view=view), want[layer], f"{what}: {layer} records")
        ids, cov = r.read_cryptomatte(layer, view=view)
        wids, wcov = R.rank(want[layer])
        assert_same(ids, wids, f"{what}: {layer} ids")
        assert_same(cov, wcov, f"{what}: {layer} coverage")


STATS = ("total_frames", "rays_total", "rays_closest_total", "rays_shadow_total", "rays_primary_total", "updates_rendered")


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_scenes(halart, oracle, seed):
    from random_scenes import random_scene
    s, env, kw = random_scene(seed)
    r, off = make(halart, s, kw, env), make(halart, s, kw, env, layers=None)
    try:
        for frames in (1, 2):
            r.update_batch(frames); off.update_batch(frames)
        check(r, R.records(oracle, s, kw["width"], kw["height"], 3), f"seed {seed}")
        for k in range(4):
            assert_same(r.read_image(k), off.read_image(k), f"seed {seed}: image {k}")
        a, b = r.statistics(), off.statistics()
        assert [getattr(a, f) for f in STATS] == [getattr(b, f) for f in STATS]
    finally:
        r.close(); off.close()


def textured_scene(w=W, h=H, cameras=1):
    s = scenes.bunny_class(subdivisions=4, aspect=w / h, disney=True)
    scenes.attach_textures(s, sets=1, size=64)
    if cameras > 1:
        s = scenes.with_extra_cameras(s, cameras - 1)
    return s, scenes.sky_sun_envmap(128, 64, sun_gain=300.0)


@gpu
def test_images_0_5_unchanged_and_update_batch_equals_updates(halart, oracle):
    s, env = textured_scene()
    kw = kw_of(md=4, rr=2, tm=(True, True, False))
    on = make(halart, s, kw, env, aovs=(True, True))
    off = make(halart, s, kw, env, aovs=(True, True), layers=None)
    single = make(halart, s, kw, env, layers=("object", "asset"))
    try:
        for x in (on, off):
            x.update(); x.update_batch(2); x.update()
        for _ in range(4):
            single.update()
        for k in range(6):
            assert_same(on.read_image(k), off.read_image(k), f"image {k}")
        want = R.records(oracle, s, W, H, 4)
        check(on, want, "textured")
        check(single, want, "single updates", layers=("object", "asset"))
        with pytest.raises(halart.HalaRendererError, match="layer is off"):
            single.read_cryptomatte("material")
    finally:
        on.close(); off.close(); single.close()


@gpu
@pytest.mark.parametrize("seed", [9, 17])
def test_two_level_trees(halart, oracle, seed):
    from random_scenes import random_scene
    oracle.set_instancing(True)
    try:
        s, env, kw = random_scene(seed, instances=True)
        r = make(halart, s, kw, env, build=dict(instancing=True))
        try:
            assert r.bvh_info().instance_ref_count > 0
            r.update(); r.update()
            check(r, R.records(oracle, s, kw["width"], kw["height"], 2), f"two-level seed {seed}")
        finally:
            r.close()
    finally:
        oracle.set_instancing(False)


@gpu
def test_views_equal_single_view_renders(halart, oracle):
    views = [2, 0, 1, 2]
    scene = scenes.with_extra_cameras(scenes.cornell_box(aspect=W / H), 2)
    r = make(halart, scene, kw_of())
    try:
        r.set_views(views)
        r.update(); r.update_batch(2)
        for v, c in enumerate(views):
            check(r, R.records(oracle, scenes.swap_cameras(scene, c), W, H, 3), f"view {v}", view=v)
        with pytest.raises(halart.HalaRendererError, match="does not exist"):
            r.read_cryptomatte("object", view=4)
    finally:
        r.close()


@gpu
def test_adaptive_sampling(halart, oracle):
    scene = scenes.cornell_box(aspect=W / H)
    r = make(halart, scene, kw_of())
    try:
        r.set_adaptive_sampling(0.2, min_samples=2, interval=2)
        r.set_cryptomatte()
        frames, snap = 0, None
        for batch in (2, 2, 2, 3, 3):
            r.update_batch(batch)
            frames += batch
            rec = r.read_cryptomatte_records("object")
            if snap is not None:  # pixels of blocks that had converged before this batch keep their records
                done = snap[0] < frames - batch
                assert np.array_equal(rec[done], snap[1][done])
            snap = (r.read_sample_counts(), rec)
        counts = snap[0]
        assert counts.min() < frames, "no block converged"
        assert np.array_equal(snap[1][..., 0], counts)  # n stops with the block
        every = R.records(oracle, scene, W, H, frames, snapshots=True)
        for layer in R.LAYERS:
            got = r.read_cryptomatte_records(layer)
            for n in np.unique(counts):
                sel = counts == n
                assert np.array_equal(got[sel], every[int(n) - 1][layer][sel]), (layer, n)
    finally:
        r.close()


def play(halart, timing_period, fusion):
    s, env = textured_scene()
    r = make(halart, s, kw_of(md=4, rr=2, tm=(True, True, False)), env)
    out = []
    try:
        r.set_pass_fusion(fusion)
        r.set_launch_timing_period(timing_period)
        for frames in (1, 2, 1):
            r.update_batch(frames)
            r.render()
            out += [r.read_cryptomatte_records(layer) for layer in R.LAYERS]
        r.set_cryptomatte(("material",))
        r.update(); r.update()
        out += [r.read_cryptomatte_records("material")] + [r.read_image(k) for k in range(4)]
    finally:
        r.close()
    return out


@gpu
def test_pass_fusion_and_tail_overlap(halart):
    ref = play(halart, 1, 0)  # serial: timed updates, one launch per pass
    for period, fusion in ((0, 1), (0, 2), (1, 2)):
        got = play(halart, period, fusion)
        assert len(got) == len(ref)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert a.tobytes() == b.tobytes(), (period, fusion, i)


@gpu
def test_refit_after_a_scene_edit(halart, oracle):
    import scene_edits as E
    base = E.cornell()
    fwd, _ = E.edit_ops("E1-move-mesh-node", base.scene)
    edited = E.apply_to_scene(base.scene, fwd)
    kw = dict(base.kw)
    r = make(halart, base.scene, kw, base.env)
    try:
        r.update_batch(3)
        before = R.records(oracle, base.scene, kw["width"], kw["height"], 3)
        check(r, before, "before the edit")
        E.apply_to_renderer(r, fwd)
        r.refit()
        with pytest.raises(halart.HalaRendererError, match="update first"):
            r.read_cryptomatte("object")
        r.update(); r.update()
        after = R.records(oracle, edited, kw["width"], kw["height"], 2)
        check(r, after, "after the refit")
        assert after["object"].tobytes() != before["object"].tobytes()
    finally:
        r.close()


def tiles_scene(n=20, size=9.0, pitch=10.0):
    """the Cornell box with n x n small quads of distinct nodes (each under a parent of its row, each row's material its own) in front of
    the camera: at a few pixels per frame every pixel sees far more than seven objects"""
    import hala_renderer_amd as H
    s = scenes.cornell_box(aspect=1.0)
    tile = scenes._merge_quads([((0, 0, 0), (size, 0, 0), (size, size, 0), (0, size, 0))])
    tile.material_index = 0
    s.meshes.append(H.HalaMesh([tile]))
    m = len(s.meshes) - 1
    for j in range(n):
        s.materials.append(H.HalaMaterial(type=H.HalaMaterialType.DIFFUSE, base_color=(0.2 + 0.03 * j, 0.5, 0.5), roughness=0.0))
        row = len(s.nodes)
        t = np.eye(4, dtype=f32)
        t[:3, 3] = (278.0 - 0.5 * n * pitch, 273.0 - 0.5 * n * pitch + j * pitch, 100.0)
        s.nodes.append(H.HalaNode(name=f"row{j}", local_transform=t))
        for i in range(n):
            ti = np.eye(4, dtype=f32)
            ti[0, 3] = i * pitch
            s.nodes.append(H.HalaNode(name=f"tile{j}_{i}", parent=row, mesh_index=m, local_transform=ti))
    return s


@gpu
def test_many_small_objects_overflow_into_other(halart, oracle):
    s = tiles_scene()
    kw = kw_of(w=5, h=4, md=2, rr=1)
    r = make(halart, s, kw)
    try:
        r.update_batch(12); r.update_batch(12)
        want = R.records(oracle, s, 5, 4, 24)
        assert want["object"][..., 1].max() > 0
        check(r, want, "tiles")
    finally:
        r.close()


@gpu
def test_manifest_save_and_matte(halart, oracle, tmp_path):
    s = scenes.cornell_box(aspect=W / H)
    s.nodes[1].name = 'short "block" \\ café'
    s.nodes[2].name = ""  # node2
    names = ["white", None, "grün\n", "", "block"]
    r = make(halart, s, kw_of(), names=names)
    try:
        r.update_batch(3)
        want = R.records(oracle, s, W, H, 3, names=names)
        check(r, want, "named")
        for layer in R.LAYERS:
            assert r.cryptomatte_manifest(layer) == R.manifest(s, layer, names), layer
        m = r.cryptomatte_manifest("object")
        assert 'short "block" \\ café' in m and "node2" in m and "room" in m
        path = tmp_path / "crypto.exr"
        r.save_cryptomatte(path)
        chans, attrs, planes = read_exr(path)
        assert chans == sorted(chans) and chans[:2] == ["A", "B"]
        accum = r.read_image(0)
        for c, nm in enumerate("RGBA"):
            assert planes[nm].tobytes() == accum[..., c].tobytes(), nm
        for layer, lname in zip(R.LAYERS, R.LAYER_NAMES):
            ids, cov = r.read_cryptomatte(layer)
            for k in range(3):
                for c, ch in enumerate("RGBA"):
                    src = (ids if c % 2 == 0 else cov)[..., 2 * k + c // 2]
                    assert planes[f"{lname}0{k}.{ch}"].tobytes() == src.tobytes(), (lname, k, ch)
            key = R.layer_key(lname)
            assert attrs[f"cryptomatte/{key}/name"][1] == lname.encode()
            assert attrs[f"cryptomatte/{key}/hash"][1] == b"MurmurHash3_32"
            assert attrs[f"cryptomatte/{key}/conversion"][1] == b"uint32_to_float32"
            assert json.loads(attrs[f"cryptomatte/{key}/manifest"][1].decode("utf-8")) == r.cryptomatte_manifest(layer)
        ids, cov = r.read_cryptomatte("object")
        matte = halart.cryptomatte_matte(ids, cov, m, ["room"])
        wids, wcov = R.rank(want["object"])
        sel = (wids.view(u32) == int(m["room"], 16)) & (wcov > 0)
        twin = np.zeros((H, W), f32)
        for k in range(6):
            twin = (twin + np.where(sel[..., k], wcov[..., k], f32(0))).astype(f32)
        assert matte.tobytes() == twin.tobytes() and 0 < matte.max() <= 1
    finally:
        r.close()


@gpu
def test_refusals_leave_the_renderer_as_it_was(halart):
    scene = scenes.cornell_box(aspect=W / H)
    r = make(halart, scene, kw_of(), layers=None)
    lib = halart.load_library()
    try:
        def frame(n=2):
            r.reset_accumulation()
            r.update_batch(n)
            return [r.read_image(k).tobytes() for k in range(4)]

        before = frame()
        for kw in (dict(mask=0), dict(mask=8), dict(null_names=True)):
            d, keep = descriptor(halart, **kw)
            with pytest.raises(halart.HalaRendererError):
                halart.check(lib.hala_rt_set_cryptomatte(r._h, C.byref(d)))
        with pytest.raises(halart.HalaRendererError, match="off"):
            r.read_cryptomatte("object")
        with pytest.raises(halart.HalaRendererError, match="off"):
            r.cryptomatte_manifest("object")
        assert frame() == before
        r.set_cryptomatte(("object", "asset"))
        assert r.statistics().total_frames == 0
        with pytest.raises(halart.HalaRendererError, match="update first"):
            r.read_cryptomatte_records("object")
        r.update_batch(2)
        rec = r.read_cryptomatte_records("object")
        with pytest.raises(halart.HalaRendererError, match="layer is off"):
            r.read_cryptomatte("material")
        with pytest.raises(halart.HalaRendererError, match="does not exist"):
            r.read_cryptomatte_records("object", view=1)
        with pytest.raises(halart.HalaRendererError, match="sharded"):
            r.set_tile_shard(0, 2, 16)
        d, keep = descriptor(halart, mask=9)
        with pytest.raises(halart.HalaRendererError):
            halart.check(lib.hala_rt_set_cryptomatte(r._h, C.byref(d)))
        assert r.statistics().total_frames == 2 and r.read_cryptomatte_records("object").tobytes() == rec.tobytes()
        assert [r.read_image(k).tobytes() for k in range(4)] == before
        r.set_cryptomatte(None)
        with pytest.raises(halart.HalaRendererError, match="off"):
            r.read_cryptomatte_records("object")
        assert frame() == before
        r.set_tile_shard(0, 2, 16)
        with pytest.raises(halart.HalaRendererError, match="sharded"):
            r.set_cryptomatte()
    finally:
        r.close()
