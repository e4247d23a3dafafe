#!/usr/bin/env python3
"""Is the gfx950 device code of every csrc/*.hip the same at two revisions?  Each unit is compiled device-only to assembly text with the
product's flags (build.FLAGS, the unit's UNIT_FLAGS) and the two texts are compared byte for byte.  Host code that names a template's
instantiations in another order makes the compiler emit the same kernels in another order, with other function numbers in their local labels:
a unit whose text differs is therefore compared kernel by kernel (same_code), and "same kernels, same code (order differs)" is reported apart
from a real difference.  A unit that really differs gets a per-kernel summary of what decides occupancy -- vector registers, scratch, LDS --
and of the instruction count, old against new.  No GPU is needed.
usage: isa_identity.py [OLD [NEW]]   (git revisions; default HEAD~1 against the working tree).  Exit status 0 only if every unit is
byte-identical or same-code."""
import concurrent.futures
import io
import os
import re
import shutil
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from palettenerf_amd import build  # noqa: E402


def checkout(rev, tmp):
    """The tree whose units get compiled: ROOT itself for the working tree, else `rev`'s sources unpacked under tmp."""
    if rev is None:
        return ROOT
    dst = os.path.join(tmp, "tree_" + rev.replace("/", "_"))
    tar = subprocess.check_output(["git", "-C", ROOT, "archive", rev, "palettenerf_amd/csrc", "include"])
    tarfile.open(fileobj=io.BytesIO(tar)).extractall(dst)
    return dst


def units(tree):
    csrc = os.path.join(tree, "palettenerf_amd", "csrc")
    return {f[:-4]: os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hip")}


def assembly(src, out):
    unit = os.path.basename(src)[:-4]
    subprocess.check_call([build.hipcc(), *build.FLAGS, *build.UNIT_FLAGS.get(unit, []), "-fuse-cuid=none", "--cuda-device-only", "-S",
                           "-Wno-unused-command-line-argument", src, "-o", out])
    with open(out, "rb") as f:
        return f.read()


def first_difference(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    n = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
    return f"line {n + 1}: {(la[n] if n < len(la) else b'<end of file>').decode(errors='replace').strip()!r} -> {(lb[n] if n < len(lb) else b'<end of file>').decode(errors='replace').strip()!r}"


# a local label carries the number of its function within the unit (.LBB3_2: block 2 of function 3), which moves when the emission order does
LOCAL_LABEL = re.compile(rb"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+")


def kernel_code(text):
    """{kernel symbol: its code} of one unit's assembly text.  A kernel's code is the text from its label to the .end_amdhsa_kernel of its
    descriptor (instructions, jump tables, every .amdhsa_ field) without `;` comments and blank lines, the function number of local labels
    replaced by a placeholder."""
    lines = text.split(b"\n")
    label = {m.group(1): i for i, ln in enumerate(lines) if (m := re.match(rb"(\w+):", ln))}
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(rb"\s*\.amdhsa_kernel (\w+)", ln)
        if not m or m.group(1) not in label:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == b".end_amdhsa_kernel")
        body = (LOCAL_LABEL.sub(rb".\1#", ln.split(b";")[0]).rstrip() for ln in lines[label[m.group(1)]:end + 1])
        out[m.group(1).decode()] = b"\n".join(ln for ln in body if ln.strip())
    return out


def same_code(old_text, new_text):
    """(True, []) if both texts hold the same kernels with the same code, else (False, [what differs, one line per kernel])."""
    old, new = kernel_code(old_text), kernel_code(new_text)
    why = [f"only in old: {k}" for k in sorted(set(old) - set(new))] + [f"only in new: {k}" for k in sorted(set(new) - set(old))]
    why += [f"{k}: " + first_difference(old[k], new[k]) for k in sorted(set(old) & set(new)) if old[k] != new[k]]
    return not why, why


FIELDS = ("next_free_vgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(text):
    """{kernel: (VGPRs, scratch bytes, LDS bytes, instructions)} of one unit's assembly text: the three .amdhsa_ fields of the kernel's
    descriptor block and the instruction lines between the kernel's label and that block."""
    lines = text.decode(errors="replace").split("\n")
    label = {m.group(1): i for i, ln in enumerate(lines) if (m := re.match(r"(\w+):\s", ln))}
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\w+)", ln)
        if not m or m.group(1) not in label:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        desc = dict(ln.split()[:2] for ln in lines[i + 1:end] if len(ln.split()) >= 2)
        body = sum(1 for ln in lines[label[m.group(1)] + 1:i] if re.match(r"\s+[a-z]\w*(\s|$)", ln))
        out[m.group(1)] = tuple(int(desc[".amdhsa_" + f]) for f in FIELDS) + (body,)
    return out


def demangled(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt or not names:
        return {n: n for n in names}
    plain = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, plain))


def summary(old_text, new_text):
    """One line per kernel whose resources or instruction count moved (and how many did not): VGPRs, scratch, LDS, instructions, old -> new."""
    old, new = kernels(old_text), kernels(new_text)
    names = sorted(set(old) | set(new))
    plain = demangled(names)
    same = 0
    for n in names:
        if old.get(n) == new.get(n):
            same += 1
            continue
        a, b = old.get(n), new.get(n)
        cols = [f"{x[k] if x else '-'}" for k in range(4) for x in (a, b)]
        print("    vgpr {} -> {}  scratch {} -> {}  lds {} -> {}  instructions {} -> {}  {}".format(*cols, re.sub(r"^pnr::|\(.*$", "", plain[n].replace("void ", ""))))
    print(f"    ({same} of {len(names)} kernels: same registers, scratch, LDS and instruction count)")


def main():
    old_rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD~1"
    new_rev = sys.argv[2] if len(sys.argv) > 2 else None
    with tempfile.TemporaryDirectory() as tmp:
        old, new = units(checkout(old_rev, tmp)), units(checkout(new_rev, tmp))
        with concurrent.futures.ThreadPoolExecutor(max_workers=16) as ex:
            jobs = {(side, u): ex.submit(assembly, src, os.path.join(tmp, f"{side}_{u}.s"))
                    for side, srcs in (("old", old), ("new", new)) for u, src in srcs.items()}
            text = {k: j.result() for k, j in jobs.items()}
    print(f"old: {old_rev}   new: {new_rev or 'working tree'}")
    differ = 0
    for u in sorted(set(old) | set(new)):
        if u not in old or u not in new:
            verdict = f"only in {'new' if u in new else 'old'}"
        elif text["old", u] == text["new", u]:
            verdict = "identical"
        else:
            same, why = same_code(text["old", u], text["new", u])
            n = len(kernel_code(text["new", u]))
            verdict = f"same kernels, same code (order differs; {n} kernels)" if same else "differs: " + first_difference(text["old", u], text["new", u])
        print(f"{u:16s} {verdict}")
        if verdict.startswith("differs"):
            differ += 1
            print("".join(f"    {w}\n" for w in why), end="")
            summary(text["old", u], text["new", u])
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
