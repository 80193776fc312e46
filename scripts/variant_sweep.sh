#!/bin/bash
# Compile-time constant sweep on a GPU machine (it has hipcc and rebuilds libhalart.so in ~20 s):
#   bash scripts/variant_sweep.sh "-DRT_STACK_LDS=6" "-DRT_WAVES_PER_SIMD=6" ...
# prints Mrays/s, ms/frame and the per-kernel split of bench.py (configs[3]) for the default build and for each variant (each argument
# is a set of -D flags the library is rebuilt with); the default is rebuilt at the end.
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
cd $ROOT
STEPS=${SWEEP_STEPS:-20}
SEC=${SWEEP_SECONDARY:---no-secondary}
MAKE_LOG=${TMPDIR:-/tmp}/variant_make.log
run() { timeout -k 10 300 python3 bench.py --steps $STEPS --warmup 3 --no-cpu-baseline $SEC 2>/dev/null | python3 -c "
import sys,json
b=json.loads(sys.stdin.read()); r=b['roofline']; k=r['ms_per_frame_by_kernel']; u=k['one_launch_per_pass']; f=k['fused_launches']; s=r['simt']; ub=r['unfused_kernels']['batch']
print(b['value'], b['ms_per_step'], '| per pass: closest', u['closest'], 'shade', u['shade'], 'shadow', u['shadow'], '| fused frames: primary', f['primary'], 'shade', f['shade'], 'fused', f['fused_traversal'],
      '| nodes/tris per bounce ray', ub['nodes_per_ray'], ub['tris_per_ray'],
      '| leaf passes/step @ lanes', s['closest']['leaf_passes_per_wave_step'], s['closest']['leaf_path_lanes_of_64'], s['shadow']['leaf_passes_per_wave_step'], s['shadow']['leaf_path_lanes_of_64'],
      '| node lanes', s['closest']['node_path_lanes_of_64'], s['shadow']['node_path_lanes_of_64'])
c=b.get('secondary',{}).get('configs1')
if c: print('   cornell', c['value'], c['ms_per_frame'], 'batch', c['batch_kernel']['avg_launch_ms'], 'shadow', c['shadow_kernel']['avg_launch_ms'], 'shade', c['shade_kernel']['avg_launch_ms'], '| 4K on 1 GPU', b['secondary']['configs4_on_1_gpu']['ms_per_frame'])"; }
build() { touch hala-renderer_amd/csrc/trace_closest.hip hala-renderer_amd/csrc/trace_shadow.hip hala-renderer_amd/csrc/shade.hip hala-renderer_amd/csrc/resolve.hip hala-renderer_amd/csrc/renderer.hip hala-renderer_amd/csrc/bvh_build.hip; make -C hala-renderer_amd/csrc -j16 EXTRA="$1" > "$MAKE_LOG" 2>&1 || { echo "build failed: $1"; tail -n 5 "$MAKE_LOG"; }; }
# every object depends on every header of csrc/: touching one on top rebuilds every host unit, too, with the new defines
rebuild() { touch hala-renderer_amd/csrc/hala_types.h hala-renderer_amd/csrc/bvh_sah.hip hala-renderer_amd/csrc/bvh_ploc.hip; build "$1"; }
mkdir -p gpurun_out
rebuild ""
echo "default"; run
for v in "$@"; do
  rebuild "$v"; echo "$v"; run
done
rebuild ""
