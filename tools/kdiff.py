"""dev: do two builds of a HIP object hold the same device code, kernel by kernel?
   python tools/kdiff.py PARENT.o HEAD.o [regex]
Both gfx950 code objects are disassembled and compared as text, function by function under its demangled name (so the
compilation-unit id, which differs between any two trees, plays no part).  Per kernel one of
   identical
   differs before the first matrix instruction only      (the prologue: staging, address set-up)
   differs: N lines                                      with tools/kres.py's columns of both sides
Exit status 1 when a kernel exists on one side only."""
import difflib
import re
import subprocess
import sys
import tempfile

from kres import LLVM, demangle, resources, unbundle


def functions(co):
    """{demangled name: [instruction text, ...]} of a code object"""
    txt = subprocess.check_output([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    heads, bodies = [], []
    for line in txt.split("\n"):
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
        if m:
            heads.append(m.group(1))
            bodies.append([])
        elif bodies and line.startswith(("\t", " ")) and line.strip():
            bodies[-1].append(re.sub(r"\s*//.*", "", line).strip())
    return dict(zip(demangle(heads), bodies))


def first_matrix(lines):
    return next((i for i, l in enumerate(lines) if l.startswith("v_mfma")), len(lines))


def differing_lines(a, b):
    lo = 0
    while lo < min(len(a), len(b)) and a[lo] == b[lo]:
        lo += 1
    hi = 0
    while hi < min(len(a), len(b)) - lo and a[-1 - hi] == b[-1 - hi]:
        hi += 1
    a, b = a[lo:len(a) - hi], b[lo:len(b) - hi]
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")


def compare(parent_obj, head_obj, pat="."):
    """[{kernel, verdict, and for a kernel that differs: lines, parent, head (kres columns)}]"""
    side = []
    for obj in (parent_obj, head_obj):
        with tempfile.TemporaryDirectory() as tmp:
            try:
                co = unbundle(obj, tmp)
            except subprocess.CalledProcessError:      # host code only (capi.o): no kernels to compare
                side.append(({}, {}))
                continue
            side.append((functions(co), resources(co)))
    (fp, rp), (fh, rh) = side
    out = []
    for nm in sorted(set(fp) | set(fh)):
        if not re.search(pat, nm):
            continue
        if nm not in fp or nm not in fh:
            out.append({"kernel": nm, "verdict": "only in " + ("head" if nm in fh else "parent")})
            continue
        a, b = fp[nm], fh[nm]
        if a == b:
            out.append({"kernel": nm, "verdict": "identical"})
            continue
        ma, mb = first_matrix(a), first_matrix(b)
        row = {"kernel": nm, "parent": rp.get(nm, "?"), "head": rh.get(nm, "?")}
        if ma < len(a) and a[ma:] == b[mb:]:
            row["verdict"] = "differs before the first matrix instruction only"
            row["lines"] = differing_lines(a[:ma], b[:mb])
        else:
            row["verdict"] = "differs"
            row["lines"] = differing_lines(a, b)
        out.append(row)
    return out


def main():
    rows = compare(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else ".")
    for r in rows:
        if r["verdict"] == "differs":
            print(f"differs: {r['lines']} lines  {r['kernel']}\n    parent {r['parent']}\n    head   {r['head']}")
        else:
            print(f"{r['verdict']}  {r['kernel']}")
    sys.exit(1 if any(r["verdict"].startswith("only in") for r in rows) else 0)


if __name__ == "__main__":
    main()
