"""Rig — a hala_rig_desc (docs/RENDER_SPEC.md 19) seen from Python: the skins, morph targets and clips of a glTF file as numpy
arrays, and sample_clip(), the host-side evaluation of a clip at a time (hala_rig_sample_clip: no renderer, no GPU).  A Rig borrows
the arrays of the NativeScene it came from and keeps that scene alive."""
import ctypes as C

import numpy as np

from . import _abi as A

INVALID = 0xFFFFFFFF


def _array(ptr, shape, dtype):
    n = int(np.prod(shape))
    if not ptr or n == 0:
        return None if not ptr else np.zeros(shape, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype).reshape(shape).copy()


class Rig:
    def __init__(self, desc_ptr, owner=None):
        self._ptr, self._owner = desc_ptr, owner
        d = self.desc = desc_ptr.contents
        self.node_count, self.weight_floats, self.palette_floats = d.node_count, d.weight_floats, d.palette_floats
        self.nodes = [dict(parent=n.parent, is_matrix=bool(n.is_matrix), local_transform=np.array(n.local_transform[:], dtype=np.float32),
                           translation=np.array(n.translation[:], dtype=np.float32), rotation=np.array(n.rotation[:], dtype=np.float32),
                           scale=np.array(n.scale[:], dtype=np.float32)) for n in (d.nodes[k] for k in range(d.node_count))]
        self.node_of_gltf = [d.node_of_gltf[k] for k in range(d.gltf_node_count)]
        self.skins = [dict(joints=[s.joints[j] for j in range(s.joint_count)], inverse_bind_matrices=_array(s.inverse_bind_matrices, (s.joint_count, 16), np.float32))
                      for s in (d.skins[k] for k in range(d.skin_count))]
        self.bindings = []
        for b in (d.bindings[k] for k in range(d.binding_count)):
            shape = (b.target_count, b.vertex_count, 3)
            self.bindings.append(dict(
                mesh_index=b.mesh_index, primitive_index=b.primitive_index, node=b.node, node_count=b.node_count, skin=None if b.skin == INVALID else b.skin,
                vertex_count=b.vertex_count, influence_sets=b.influence_sets, target_count=b.target_count,
                joint_count=0 if b.skin == INVALID else d.skins[b.skin].joint_count,
                joints=_array(b.joints, (b.vertex_count, 4), np.uint16), weights=_array(b.weights, (b.vertex_count, 4), np.float32),
                targets=_array(b.target_position_deltas, shape, np.float32), normal_targets=_array(b.target_normal_deltas, shape, np.float32),
                tangent_targets=_array(b.target_tangent_deltas, shape, np.float32), default_weights=_array(b.default_weights, (b.target_count,), np.float32),
                weight_first=b.weight_first, palette_first=b.palette_first))
        self.clips = []
        for c in (d.clips[k] for k in range(d.clip_count)):
            samplers = []
            for s in (c.samplers[k] for k in range(c.sampler_count)):
                per_key = s.width * (3 if s.interpolation == A.RIG_CUBICSPLINE else 1)
                samplers.append(dict(times=_array(s.times, (s.key_count,), np.float32), values=_array(s.values, (s.key_count, per_key), np.float32),
                                     interpolation=s.interpolation, width=s.width))
            channels = [dict(sampler=ch.sampler, node=ch.node, path=ch.path) for ch in (c.channels[k] for k in range(c.channel_count))]
            self.clips.append(dict(name=(c.name or b"").decode(errors="replace"), samplers=samplers, channels=channels, time_first=c.time_first,
                                   time_last=c.time_last))

    def desc_ptr(self):
        return self._ptr

    def unpack(self, locals_, weights, palettes):
        """the packed outputs of hala_rig_sample_clip / hala_rt_get_rig_pose -> dict(locals [N, 4, 4] as update_node_transform takes
        them, weights and palettes: one entry per binding, None where the binding has no targets / no skin)"""
        out = dict(locals=locals_.reshape(-1, 4, 4).transpose(0, 2, 1).copy(), weights=[], palettes=[])
        for b in self.bindings:
            out["weights"].append(weights[b["weight_first"]:b["weight_first"] + b["target_count"]].copy() if b["target_count"] else None)
            out["palettes"].append(palettes[b["palette_first"]:b["palette_first"] + 12 * b["joint_count"]].reshape(-1, 3, 4).copy() if b["joint_count"] else None)
        return out

    def buffers(self):
        return (np.zeros(self.node_count * 16, dtype=np.float32), np.zeros(self.weight_floats, dtype=np.float32),
                np.zeros(self.palette_floats, dtype=np.float32))


def clip_index(clip):
    return INVALID if clip is None else int(clip)


def sample_clip(rig: Rig, clip, time):
    """the pose of clip `clip` (None: the file's own pose) at `time` -> Rig.unpack()'s dict.  Host code only"""
    from . import check, load_library
    fp = C.POINTER(C.c_float)
    l, w, p = rig.buffers()
    check(load_library().hala_rig_sample_clip(rig.desc_ptr(), C.c_uint32(clip_index(clip)), C.c_float(time), l.ctypes.data_as(fp), w.ctypes.data_as(fp),
                                               p.ctypes.data_as(fp)))
    return rig.unpack(l, w, p)
