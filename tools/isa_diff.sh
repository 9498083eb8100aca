#!/bin/bash
# Proves that a source cleanup left the device code alone: compiles every lfbm5d_amd/csrc/*.hip of a base commit and of the working
# tree to gfx950 assembly and compares them kernel by kernel (instruction text and the .amdhsa_* descriptor block: registers, LDS,
# scratch, occupancy).  No GPU needed.
#   tools/isa_diff.sh <base-commit> ['old=new' ...]
# The base commit's lfbm5d_amd/csrc and include are exported with `git archive` into a temporary directory; nothing is checked out
# in the working tree.  Each file is compiled with the flags its own tree's Makefile gives it (`make -n`), with -c replaced by
# --offload-device-only -S -fuse-cuid=none (without the last, two compilations of one file differ in the __hip_cuid_* symbol).
# 'old=new' pairs name kernels that were renamed on purpose, as demangled names without return type and parameter list, e.g.
#   tools/isa_diff.sh HEAD~1 'k_group_dct8<1>=k_group_dct8'
# Their bodies are compared under that mapping.  Exit status 0: the symbol sets are equal (up to the renames) and every kernel matches.
# ISA_DIFF_WORK=<dir> keeps the assembly there (and reuses a base tree already compiled into it) instead of a temporary directory.
set -euo pipefail
[ $# -ge 1 ] || { sed -n '2,13p' "$0"; exit 2; }
root=$(cd "$(dirname "$0")/.." && pwd)
base=$(git -C "$root" rev-parse --verify "$1^{commit}"); shift
if [ -n "${ISA_DIFF_WORK:-}" ]; then work=$ISA_DIFF_WORK; mkdir -p "$work"; else work=$(mktemp -d); trap 'rm -rf "$work"' EXIT; fi

# compile_tree <tree root> <assembly directory>
compile_tree() {
  local csrc=$1/lfbm5d_amd/csrc out=$2 f cmd
  mkdir -p "$out"
  for f in "$csrc"/*.hip; do
    f=$(basename "$f" .hip)
    cmd=$(make -n -B -C "$csrc" "$f.o" | grep -- "-c $f\.hip" | head -1)
    [ -n "$cmd" ] || { echo "isa_diff: no compile rule for $f.hip in $csrc/Makefile" >&2; return 1; }
    cmd=${cmd/ -c / --offload-device-only -S -fuse-cuid=none }
    echo "cd '$csrc' && ${cmd% -o *} -o '$out/$f.s'"
  done | xargs -P "${JOBS:-$(nproc)}" -d '\n' -n 1 bash -c
}

if [ ! -f "$work/base_$base/done" ]; then
  mkdir -p "$work/base_$base/tree"
  git -C "$root" archive "$base" lfbm5d_amd/csrc include | tar -x -C "$work/base_$base/tree"
  compile_tree "$work/base_$base/tree" "$work/base_$base/asm"
  touch "$work/base_$base/done"
fi
rm -rf "$work/new"
compile_tree "$root" "$work/new"

python3 - "$work/base_$base/asm" "$work/new" "$@" <<'EOF'
import glob, os, re, shutil, subprocess, sys

def demangle(names):
    out = subprocess.run([shutil.which("llvm-cxxfilt") or "c++filt"],
                         input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))

def short(d):
    """demangled name without return type and parameter list: 'void k<1>(Args)' -> 'k<1>'"""
    d = d.replace("(anonymous namespace)::", "")
    depth, end = 0, len(d)
    for i, c in enumerate(d):                       # the parameter list opens at the first '(' outside template brackets
        if c == '<': depth += 1
        elif c == '>': depth -= 1
        elif c == '(' and depth == 0: end = i; break
    head, depth = d[:end], 0
    for i in range(len(head) - 1, -1, -1):          # the return type ends at the last blank outside template brackets
        if head[i] == '>': depth += 1
        elif head[i] == '<': depth -= 1
        elif head[i] == ' ' and depth == 0: return head[i + 1:]
    return head

LABEL = re.compile(r'(\.L[A-Za-z_]+?)\d+(_\d+)?\b')   # .LBB<n>_<m>, .Lfunc_end<n>, .LJTI<n>_<m>: <n> is the function's index in its file

def functions(path):
    """{symbol: normalised text} for every function symbol of one assembly file, its kernel descriptor included"""
    lines = open(path).read().split("\n")
    syms = [m.group(1) for l in lines if (m := re.match(r'\s*\.type\s+(\S+),@function', l))]
    res, cur = {}, None
    for l in lines:
        m = re.match(r'(\S+):', l)
        if m and m.group(1) in syms: cur = m.group(1); res[cur] = []; continue
        if cur is None: continue
        if re.match(r'\s*\.size\s+' + re.escape(cur) + ',', l): cur = None; continue
        l = l.split(';')[0].rstrip()
        if l: res[cur].append(LABEL.sub(lambda m: m.group(1) + (m.group(2) or ''), l).replace(cur, '@SELF'))
    return {s: "\n".join(t) for s, t in res.items()}

def tree(d):
    res = {}
    for p in sorted(glob.glob(os.path.join(d, "*.s"))):
        fn = functions(p)
        dm = demangle(list(fn)) if fn else {}
        for s, t in fn.items(): res[(os.path.basename(p)[:-2], short(dm[s]))] = t
    return res

old, new = tree(sys.argv[1]), tree(sys.argv[2])
renames = dict(a.split('=', 1) for a in sys.argv[3:])
unused = set(renames) - {n for _, n in old}
old = {(f, renames.get(n, n)): (n, t) for (f, n), t in old.items()}
same, differ = 0, []
for k in sorted(set(old) & set(new)):
    if old[k][1] == new[k]: same += 1
    else: differ.append(k)
gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
descr = sum('.amdhsa_kernel' in t for t in new.values())
print(f"functions compared: {same + len(differ)} ({descr} kernels with a descriptor block in the new tree), identical: {same}, different: {len(differ)}")
for f, n in sorted(k for k in old if old[k][0] != k[1]): print(f"  renamed  {f}: {old[(f, n)][0]} -> {n}")
for f, n in differ: print(f"  DIFFERS  {f}: {n}")
for f, n in gone: print(f"  ONLY IN BASE  {f}: {n}")
for f, n in added: print(f"  ONLY IN NEW   {f}: {n}")
for n in sorted(unused): print(f"  RENAME WITHOUT A BASE KERNEL  {n}")
sys.exit(1 if differ or gone or added or unused else 0)
EOF
