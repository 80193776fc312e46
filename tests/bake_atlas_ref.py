"""The float32 numpy twin of bake atlases (docs/RENDER_SPEC.md 4.12): bake_ref.Twin with the chart of each triangle's instance between the
UVs and the corners, by brute force: every triangle of every charted instance against every texel of the atlas.

    atlas = Atlas(twin, charts)                      # twin: a bake_ref.Twin of the scene; charts: [(instance, scale, offset, flags)]
    owner = atlas.owners(W, H)                       # [H * W] uint32: the lowest covering global id over ALL charted instances, MISS: none
    samples, texels = atlas.samples(W, H, ...)       # A.OCCLUSION_SAMPLE_DTYPE and A.BAKE_TEXEL_DTYPE, [H * W] each; normals by each chart's flags
    table = atlas.table()                            # the charts as A.BAKE_CHART_DTYPE, what HalaRenderer.bake_atlas_* takes

A corner is fma(uv, scale, offset) * (W, H): one fma (aov_ref.fma, rounded once), then one rounded product, per component.  Everything
behind the corners is bake_ref's, unchanged: the edge function, the coverage rule, the barycentrics, point, normal and the records; the
dilation is bake_ref.dilate and the occlusion records are occlusion_ref's reduction of an any-hit trace of the samples, texel i being
sample i."""
import numpy as np

import bake_ref as BR
import hala_renderer_amd as H
from aov_ref import fma

f32 = np.float32
A = H._abi
MISS = BR.MISS


class Atlas(BR.Twin):
    def __init__(self, twin, charts):
        self.__dict__.update(twin.__dict__)  # the scene's records, shared and never written
        t = len(self.uv)
        self.charts = [(int(i), (f32(s[0]), f32(s[1])), (f32(o[0]), f32(o[1])), int(fl)) for i, s, o, fl in charts]
        self.scale, self.offset = np.zeros((t, 2), f32), np.zeros((t, 2), f32)
        self.flags, self.charted = np.zeros(t, np.uint32), np.zeros(t, bool)
        for i, s, o, fl in self.charts:
            lo, hi = int(self.first[i]), int(self.first[i + 1])
            assert not self.charted[lo:hi].any(), "an instance has one chart"
            self.scale[lo:hi], self.offset[lo:hi], self.flags[lo:hi], self.charted[lo:hi] = s, o, fl, True

    def table(self):
        t = np.zeros(len(self.charts), dtype=A.BAKE_CHART_DTYPE)
        for k, (i, s, o, fl) in enumerate(self.charts):
            t[k] = (i, fl, s, o)
        return t

    def corners(self, ids, W, H, dt=f32):
        """the atlas corners of triangles `ids` in texel units: fma(uv, scale, offset), then one float32 product with (W, H)"""
        with np.errstate(all="ignore"):
            a = fma(self.uv[ids], self.scale[ids][:, None, :], self.offset[ids][:, None, :]).astype(f32)
            t = (a * np.array([W, H], f32)).astype(f32).astype(dt)
        return [(t[:, c, 0], t[:, c, 1]) for c in range(3)]

    def owners(self, W, H, chunk=512):
        """[H * W] uint32: the lowest global id among the triangles of all charted instances that cover the texel's centre, MISS: none"""
        px, py = BR.centres(W, H)
        owner = np.full(W * H, MISS, dtype=np.uint32)
        every = np.nonzero(self.charted)[0]
        for a in range(0, len(every), chunk):
            ids = every[a:a + chunk]
            area, w0, w1, w2 = self.edge_values(ids, W, H, px, py)
            cov = BR.covers(area[:, None], w0, w1, w2)
            owner = np.minimum(owner, np.where(cov, ids[:, None].astype(np.uint32), np.uint32(MISS)).min(axis=0))
        return owner

    def samples(self, W, H, bias=0.0, reach=np.inf, owner=None):
        """(samples, texels) [H * W]: RENDER_SPEC 4.11's sample and texel record of every texel, the normal by the flags of its owner's chart"""
        owner = self.owners(W, H) if owner is None else owner
        own_flags = np.where(owner != MISS, self.flags[np.where(owner != MISS, owner, 0).astype(np.int64)], np.uint32(MISS))
        samples = texels = None
        for fl in sorted(set(c[3] for c in self.charts)):
            s, t = BR.Twin.samples(self, None, W, H, flags=fl, bias=bias, reach=reach, owner=owner)
            if samples is None:
                samples, texels = s, t  # (the texel records do not depend on the flags)
            else:
                m = own_flags == fl
                samples[m] = s[m]
        return samples, texels
