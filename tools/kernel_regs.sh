#!/bin/bash
# Register / scratch usage of the group and aggregation kernels (cross-compile, no GPU needed).
# Also kept under it: lfbm5d_view.hip (k_view_sweep, k_view_sweep_subpel, k_view_sweep_occl: no scratch and no spills in any; the
# holding instantiations must stay at or under 128 VGPRs, four workgroups per CU; "spill" is the vector, "sgpr-spill" the scalar spill
# count, and both must be 0), lfbm5d_consist.hip, lfbm5d_clip.hip, lfbm5d_photo.hip, lfbm5d_pgclip.hip, lfbm5d_repair.hip (k_repair_sweep: no scratch, no spills).
cd "$(dirname "$0")/../lfbm5d_amd/csrc"
f=${1:-lfbm5d_group_ht.hip}
extra=""; [ "$f" = lfbm5d_bm.hip -o "$f" = lfbm5d_scan2.hip -o "$f" = lfbm5d_clip.hip -o "$f" = lfbm5d_photo.hip -o "$f" = lfbm5d_pgclip.hip -o "$f" = lfbm5d_repair.hip ] && extra="-ffp-contract=off"
hipcc -O3 --offload-arch=gfx950 -std=c++17 $extra -S --cuda-device-only -o /tmp/kregs.s $f 2>&1 | grep -E "error" -A3
python3 - <<'PY'
import re
t=open('/tmp/kregs.s').read()
for b in t.split('  - .agpr_count')[1:]:
    g=lambda k: re.search(r'\.%s:\s+(\S+)'%k,b).group(1)
    print('%-60s vgpr %3s sgpr %3s spill %s sgpr-spill %s scratch %s lds %s'%(g('name')[22:80],g('vgpr_count'),g('sgpr_count'),g('vgpr_spill_count'),g('sgpr_spill_count'),g('private_segment_fixed_size'),g('group_segment_fixed_size')))
PY
