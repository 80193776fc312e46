#!/bin/bash
# Per-kernel resource table of a built libhalart*.so: VGPRs, SGPRs, scratch (private segment) bytes per lane, static LDS, spills, workgroup
# size, and the kernel's instruction count with a hash of its instruction text (llvm-objdump -d --no-show-raw-insn, the trailing
# `// address` comments dropped).  Rows are sorted by name, so "which kernels did a change alter" is a diff of two outputs.
# usage: scripts/kernel_resources.sh [path/to/libhalart.so] [symbol filter regex]
LIB=${1:-hala-renderer_amd/lib/libhalart.so}
PAT=${2:-.}
TMP=$(mktemp -d)
# the fat binary holds one code object per translation unit: extract them all
python3 - "$LIB" "$TMP" <<'PY'
import sys, struct
data = open(sys.argv[1], 'rb').read()
magic = b'__CLANG_OFFLOAD_BUNDLE__'
pos = 0; n = 0
while True:
    i = data.find(magic, pos)
    if i < 0: break
    cnt = struct.unpack_from('<Q', data, i + 24)[0]
    off = i + 32
    for _ in range(cnt):
        eo, es, ts = struct.unpack_from('<QQQ', data, off); off += 24
        triple = data[off:off + ts].decode(); off += ts
        if 'gfx' in triple and es:
            open(f"{sys.argv[2]}/co{n}.elf", 'wb').write(data[i + eo:i + eo + es]); n += 1
    pos = i + 32
PY
python3 - "$TMP" "$PAT" <<'PY'
import glob, hashlib, re, subprocess, sys
LLVM = '/opt/rocm/lib/llvm/bin/'
pat = re.compile(sys.argv[2])
rows = []
for co in sorted(glob.glob(sys.argv[1] + '/co*.elf')):
    # instruction text per symbol
    text, cur = {}, None
    dis = subprocess.run([LLVM + 'llvm-objdump', '-d', '--no-show-raw-insn', '--mcpu=gfx950', co], capture_output=True, text=True).stdout
    for l in dis.split('\n'):
        m = re.match(r'^[0-9a-f]+ <(.*)>:', l)
        if m:
            cur = text.setdefault(m.group(1), [])
        elif cur is not None and l.startswith('\t'):
            cur.append(re.sub(r'\s*//.*$', '', l).strip())
    notes = subprocess.run([LLVM + 'llvm-readelf', '--notes', co], capture_output=True, text=True).stdout
    for blk in notes.split('- .agpr_count:')[1:]:
        def g(k):
            m = re.search(r'\.' + k + r':\s+(\S+)', blk); return m.group(1) if m else '?'
        insns = text.get(g('name'), [])
        while insns and insns[-1] in ('s_code_end', 's_nop 0', '...'):  # alignment padding behind the kernel: depends on what follows it
            insns.pop()
        rows.append((g('name'), g('vgpr_count'), g('sgpr_count'), g('private_segment_fixed_size'), g('group_segment_fixed_size'), g('vgpr_spill_count'),
                     g('sgpr_spill_count'), g('max_flat_workgroup_size'), str(len(insns)), hashlib.sha1('\n'.join(insns).encode()).hexdigest()[:12]))
names = subprocess.run(['/usr/bin/c++filt'], input='\n'.join(r[0] for r in rows), capture_output=True, text=True).stdout.split('\n')
out = []
for r, dem in zip(rows, names):
    dem = re.sub(r'\(.*', '', dem.strip().replace('(anonymous namespace)::', ''))
    if pat.search(dem):
        out.append(f'{dem:70s} vgpr {r[1]:>4s} sgpr {r[2]:>4s} scratch {r[3]:>5s} B  lds {r[4]:>6s} B  vspill {r[5]:>3s} sspill {r[6]:>3s} wg {r[7]:>4s} insn {r[8]:>6s} text {r[9]}')
print('\n'.join(sorted(out)))
PY
rm -rf $TMP
