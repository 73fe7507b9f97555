"""Per-kernel comparison of two hipcc -S files of one source (e.g. render_fwd.hip of the parent commit
and of the tree): every kernel's instruction sequence with comments dropped and labels renumbered in
order of first appearance.  Prints SAME / DIFFERENT / NEW / GONE per kernel.
    python tools/asm_diff.py parent.s branch.s [old-substring=new-substring ...]
A pair `old=new` compares the parent kernel whose demangled name holds `old` with the tree's kernel
whose name holds `new` (an instantiation that gained a template parameter)."""
import difflib
import re
import subprocess
import sys


def kernels(path):
    out, cur, name = {}, None, None
    for line in open(path):
        line = line.rstrip("\n")
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = cur
            cur = None
            continue
        t = re.sub(r";.*", "", line).strip()
        if t and (not t.startswith(".") or re.match(r"^\.LBB", t)):
            cur.append(t)
    return out


def norm(seq):
    m = {}
    return [re.sub(r"\.LBB\d+_\d+", lambda mo: m.setdefault(mo.group(0), f"L{len(m)}"), t) for t in seq]


def demangle(n):
    return subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().split("(gsr::Dims")[0]


def compare(na, nb, name):
    na, nb = norm(na), norm(nb)
    if na == nb:
        print("SAME     ", len(na), name)
        return
    d = [x for x in difflib.unified_diff(na, nb, lineterm="", n=0)
         if x[0] in "+-" and not x.startswith(("+++", "---"))]
    print("DIFFERENT", len(na), len(nb), f"{len(d)} changed lines", name)


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
da, db = {n: demangle(n) for n in a}, {n: demangle(n) for n in b}
paired = set()
for pair in sys.argv[3:]:
    old, new = pair.split("=", 1)
    ka = [n for n in a if old in da[n]]
    kb = [n for n in b if new in db[n]]
    assert len(ka) == 1 and len(kb) == 1, (pair, ka, kb)
    compare(a[ka[0]], b[kb[0]], f"{da[ka[0]]}  ->  {db[kb[0]]}")
    paired |= {ka[0], kb[0]}
for n in sorted(set(a) | set(b)):
    if n in paired:
        continue
    if n not in a:
        print("NEW      ", len(b[n]), db[n])
    elif n not in b:
        print("GONE     ", da[n])
    else:
        compare(a[n], b[n], da[n])
