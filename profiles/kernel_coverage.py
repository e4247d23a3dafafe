"""Which compiled kernels does the GPU suite launch?

    python profiles/kernel_coverage.py                     # the inventory: every gfx950 kernel of the product build, by unit
    python profiles/kernel_coverage.py TRACE_DIR           # ... against the kernel-trace CSV files of a `rocprofv3 --kernel-trace` run
    python profiles/kernel_coverage.py TRACE_DIR --json F  # ... and keep {name: launches} in F (the traces themselves are large and are not kept)
    python profiles/kernel_coverage.py --reduce TRACE_DIR F  # only that file, without the inventory (where the run was made, if the objects are elsewhere)
    python profiles/kernel_coverage.py --counts F          # the report from such a file

Plain Python, no GPU: inventory() reads symbol NAMES from the per-unit objects of palettenerf_amd/csrc/_obj (never the instructions), launched() reads the
profiler's CSV files.  Both spell a kernel the same way -- the demangled name without its parameter list, e.g. `pnr::k_frame_march<true, false, 1>` --
through normalise().  How the run is made and what it found: profiles/kernel_coverage/README.md."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
_ANON = "(anonymous namespace)"


def _llvm_tool(name):
    """The tool of the ROCm whose hipcc palettenerf_amd.build uses (<rocm>/bin/hipcc -> <rocm>/llvm/bin, <rocm>/lib/llvm/bin)."""
    from palettenerf_amd import build as _b
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(_b.hipcc())))
    tried = []
    for d in (os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "lib", "llvm", "bin"), os.path.join(os.path.dirname(rocm), "llvm", "bin")):
        tried.append(d)
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    raise RuntimeError(f"{name} not found under {tried}: the kernel inventory needs the LLVM tools of the ROCm toolchain")


def normalise(raw):
    """One spelling for a kernel name, whoever wrote it: readelf's `NAME.kd` after c++filt, rocprofv3's Kernel_Name column (with or without `.kd` /
    ` [clone .kd]`, with the `void ` of a template's return type and the parameter list).  The parameter list starts at the first `(` outside template
    brackets -- template arguments may hold parentheses of their own (`<(pnr::Kind)1>`)."""
    s = raw.strip().strip('"')
    for tail in (" [clone .kd]", ".kd"):
        if s.endswith(tail):
            s = s[: -len(tail)]
    if s.startswith("void "):
        s = s[5:]
    s = s.replace(_ANON, "\0")
    depth = paren = 0
    for i, c in enumerate(s):
        if c == "(":
            if depth == 0:
                s = s[:i]
                break
            paren += 1
        elif c == ")":
            paren -= 1
        elif c == "<" and paren == 0:
            depth += 1
        elif c == ">" and paren == 0:
            depth -= 1
    return s.replace("\0", _ANON).strip()


def demangle(names):
    if not names:
        return []
    out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(names)
    return out


def unit_kernels(obj, tmp):
    """Normalised names of the gfx950 kernels in one object file ([] for a unit without device code)."""
    objcopy, bundler, readelf = _llvm_tool("llvm-objcopy"), _llvm_tool("clang-offload-bundler"), _llvm_tool("llvm-readelf")
    base = os.path.basename(obj)[:-2]
    fatbin, code = os.path.join(tmp, base + ".fatbin"), os.path.join(tmp, base + ".co")
    subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fatbin, obj, os.devnull], capture_output=True, text=True)
    if not os.path.exists(fatbin) or os.path.getsize(fatbin) == 0:
        return []       # no .hip_fatbin section: host code only
    subprocess.run([bundler, "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fatbin, "--output=" + code], capture_output=True, text=True, check=True)
    syms = subprocess.run([readelf, "-sW", code], capture_output=True, text=True, check=True).stdout
    mangled = sorted({ln.split()[-1] for ln in syms.splitlines() if ln.strip().endswith(".kd")})
    return sorted({normalise(n) for n in demangle([m[:-3] for m in mangled])})


def inventory(obj_dir=None):
    """{unit: [kernel, ...]} of the product build's per-unit objects."""
    from palettenerf_amd import build as _b
    obj_dir = obj_dir or _b.OBJ
    objs = sorted(glob.glob(os.path.join(obj_dir, "*.o")))
    if not objs:
        raise RuntimeError(f"no objects under {obj_dir}: build the library first (python -m palettenerf_amd.build --force)")
    inv = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in objs:
            ks = unit_kernels(obj, tmp)
            if ks:
                inv[os.path.basename(obj)[:-2]] = ks
    return inv


def launched(trace_dir):
    """{kernel: launches} over every *kernel_trace.csv below trace_dir (pytest starts child processes: one file per process); pnr:: names only."""
    counts = {}
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = normalise(row["Kernel_Name"])
                if name.startswith("pnr::"):
                    counts[name] = counts.get(name, 0) + 1
    return counts


def report(inv, counts, out=sys.stdout):
    known = {k for ks in inv.values() for k in ks}
    total = sum(len(ks) for ks in inv.values())
    never = {u: [k for k in ks if k not in counts] for u, ks in inv.items()}
    n_never = sum(len(v) for v in never.values())
    print(f"{total} kernels compiled, {total - n_never} launched, {n_never} never launched", file=out)
    print("\nnever launched, by unit:", file=out)
    for u in sorted(never, key=lambda u: (-len(never[u]), u)):
        if never[u]:
            print(f"  {u} ({len(never[u])} of {len(inv[u])})", file=out)
            for k in never[u]:
                print(f"    {k}", file=out)
    print("\nlaunches, by unit:", file=out)
    for u in sorted(inv):
        print(f"  {u}", file=out)
        for k in inv[u]:
            if k in counts:
                print(f"    {counts[k]:>9}  {k}", file=out)
    unknown = sorted(k for k in counts if k not in known)
    print(f"\nlaunched but not in the inventory (must be empty): {len(unknown)}", file=out)
    for k in unknown:
        print(f"    {k}", file=out)
    return never, unknown


def main(argv):
    if argv and argv[0] == "--reduce":      # on the profiling machine, where the objects need not exist: traces -> {name: launches}
        counts = launched(argv[1])
        with open(argv[2], "w") as f:
            json.dump(counts, f, indent=0, sort_keys=True)
        print(f"{len(counts)} pnr:: kernels, {sum(counts.values())} launches -> {argv[2]}")
        return 0
    inv = inventory()
    if not argv:
        total = sum(len(ks) for ks in inv.values())
        for u in sorted(inv, key=lambda u: (-len(inv[u]), u)):
            print(f"{u} ({len(inv[u])})")
            for k in inv[u]:
                print(f"    {k}")
        print(f"{total} kernels in {len(inv)} units")
        return 0
    if argv[0] == "--counts":
        with open(argv[1]) as f:
            counts = json.load(f)
    else:
        counts = launched(argv[0])
        if "--json" in argv:
            with open(argv[argv.index("--json") + 1], "w") as f:
                json.dump(counts, f, indent=0, sort_keys=True)
    _, unknown = report(inv, counts)
    return 1 if unknown else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
