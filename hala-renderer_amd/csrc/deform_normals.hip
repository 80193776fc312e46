// deform_normals.hip — docs/RENDER_SPEC.md 17 "Recomputed normals": the shading normals of a posed primitive from the posed triangles
// around each vertex, and the tangent re-orthogonalised against them.  Two passes right behind k_deform on the same stream, wave64,
// 256-thread workgroups:
//
//   face pass    one lane per triangle: 12 contiguous bytes of indices, three positions (12 B each, 44 B apart in the arena), the
//                unnormalised cross product written once as a 16-B record, so that every corner of the triangle later reads the same bits.
//   vertex pass  one lane per vertex: its class, the class's range of the CSR table, the listed face records in order (one dwordx4
//                each) summed by the lane's own loop — that loop is what fixes the order of the float sum: no LDS, no atomics, no
//                reduction across lanes — then 24 B (normal + tangent) of the lane's own record.
//
// The face pass of a primitive needs every posed position of it and the vertex pass every face record: the order of the three launches on
// the stream gives both.  Every `*`, `+`, `-` is the one the spec writes, each rounded (-ffp-contract=off: no fma); `/` and sqrt are the
// correctly rounded ones, so tests/deform_normals_ref.py reproduces the vertices bit for bit.  A vertex whose sum has no usable length
// (empty list, zero, overflow, NaN from positions that overflowed) is not written at all: it keeps what k_deform wrote.
//
// Like k_deform, each pass is one launch for all the deformers of a refit that want it: a segment per deformer, a map from workgroups to
// (segment, first item), no workgroup spanning two segments, so the segment's tables are uniform over the workgroup and come in by
// scalar loads.
#include <hip/hip_runtime.h>

#include "deform.h"

namespace rt {

namespace {

#define DN_GLOBAL __attribute__((address_space(1)))
typedef float dn_f32x4 __attribute__((ext_vector_type(4)));

static_assert(sizeof(hala_vertex) == 44 && sizeof(float4) == 16, "positions are gathered at a 44-B stride, face records are 16 B");

__device__ __forceinline__ void face_pass(const NormalsTables& t, uint32_t tri) {
  const DN_GLOBAL uint32_t* idx = (const DN_GLOBAL uint32_t*)t.indices + (size_t)tri * 3u;
  const uint32_t i0 = idx[0], i1 = idx[1], i2 = idx[2];
  dn_f32x4 f = {0.0f, 0.0f, 0.0f, 0.0f};
  if (i0 < t.vertex_count && i1 < t.vertex_count && i2 < t.vertex_count) {  // (the host refuses other tables: nothing is read past the range)
    const DN_GLOBAL float* p0 = (const DN_GLOBAL float*)(t.vertices + i0);
    const DN_GLOBAL float* p1 = (const DN_GLOBAL float*)(t.vertices + i1);
    const DN_GLOBAL float* p2 = (const DN_GLOBAL float*)(t.vertices + i2);
    const float ox = p0[0], oy = p0[1], oz = p0[2];
    const float ax = p1[0] - ox, ay = p1[1] - oy, az = p1[2] - oz;
    const float bx = p2[0] - ox, by = p2[1] - oy, bz = p2[2] - oz;
    f.x = (ay * bz) - (az * by);
    f.y = (az * bx) - (ax * bz);
    f.z = (ax * by) - (ay * bx);
  }
  ((DN_GLOBAL dn_f32x4*)t.faces)[tri] = f;
}

__device__ __forceinline__ void vertex_pass(const NormalsTables& t, uint32_t v) {
  const uint32_t c = ((const DN_GLOBAL uint32_t*)t.class_of)[v];
  const DN_GLOBAL uint32_t* offsets = (const DN_GLOBAL uint32_t*)t.offsets;
  const DN_GLOBAL uint32_t* entries = (const DN_GLOBAL uint32_t*)t.entries;
  const DN_GLOBAL dn_f32x4* faces = (const DN_GLOBAL dn_f32x4*)t.faces;
  const uint32_t first = offsets[c], end = offsets[c + 1u];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (uint32_t k = first; k < end; ++k) {
    const dn_f32x4 f = faces[entries[k]];
    sx = sx + f.x; sy = sy + f.y; sz = sz + f.z;
  }
  const float q = (sx * sx + sy * sy) + sz * sz;
  if (first == end || q == 0.0f || !isfinite(q)) return;  // normal and tangent stay as k_deform wrote them
  const float len = sqrtf(q);
  const float nx = sx / len, ny = sy / len, nz = sz / len;
  DN_GLOBAL float* rec = (DN_GLOBAL float*)(t.vertices + v);
  float tx = rec[6], ty = rec[7], tz = rec[8];
  const float d = (tx * nx + ty * ny) + tz * nz;
  const float ux = tx - nx * d, uy = ty - ny * d, uz = tz - nz * d;
  const float g = (ux * ux + uy * uy) + uz * uz;
  if (g != 0.0f && isfinite(g)) {
    const float gl = sqrtf(g);
    tx = ux / gl; ty = uy / gl; tz = uz / gl;
  }
  rec[3] = nx; rec[4] = ny; rec[5] = nz;
  rec[6] = tx; rec[7] = ty; rec[8] = tz;
}

__global__ __launch_bounds__(kDeformThreads) void k_deform_faces(const NormalsTables* __restrict__ segments, const DeformBlock* __restrict__ blocks) {
  const DeformBlock b = blocks[blockIdx.x];
  const NormalsTables t = segments[b.segment];
  const uint32_t tri = b.first_vertex + threadIdx.x;  // (the block map's second word: the first triangle here)
  if (tri < t.triangle_count) face_pass(t, tri);
}

__global__ __launch_bounds__(kDeformThreads) void k_deform_vertex_normals(const NormalsTables* __restrict__ segments, const DeformBlock* __restrict__ blocks) {
  const DeformBlock b = blocks[blockIdx.x];
  const NormalsTables t = segments[b.segment];
  const uint32_t v = b.first_vertex + threadIdx.x;
  if (v < t.vertex_count) vertex_pass(t, v);
}

}  // namespace

void launch_deform_normals(const NormalsTables* segments, const DeformBlock* face_blocks, uint32_t face_block_count,
                           const DeformBlock* vertex_blocks, uint32_t vertex_block_count, hipStream_t s) {
  if (!face_block_count || !vertex_block_count) return;
  hipLaunchKernelGGL(k_deform_faces, dim3(face_block_count), dim3(kDeformThreads), 0, s, segments, face_blocks);
  hipLaunchKernelGGL(k_deform_vertex_normals, dim3(vertex_block_count), dim3(kDeformThreads), 0, s, segments, vertex_blocks);
}

}  // namespace rt
