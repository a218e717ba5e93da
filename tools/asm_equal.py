"""Is the gfx950 device code of every csrc/*.hip the same as at a git revision?  (no GPU needed)

    python tools/asm_equal.py [REV [FILE.hip ...]]        (default: HEAD, every file)
    python tools/asm_equal.py --kernels [--rename OLD=NEW ...] [REV [FILE.hip ...]]

Compiles every source of csrc/Makefile's SRCS to device assembly (the Makefile's CXXFLAGS and
per-file EXTRA flags plus --cuda-device-only -S), once as committed at REV (sources and headers
extracted into a temporary tree) and once from the working tree, blanks the __hip_cuid_<hash>
symbol (a hash of the source text) and prints per file `identical` or the first differing lines.
The assembly carries the register, LDS, spill and scratch counts of every kernel, so `identical`
for every file is "same machine code": the check for a refactor that must not change any.
Exit status 1 if any file differs.

--kernels compares kernel by kernel instead, for a change that deletes or renames some kernels of a
file and must leave the others alone.  Each file's assembly is split at `; -- Begin function SYM`
... `; -- End function` (with the function's .amdhsa_kernel block, its resource summary and its
amdhsa.kernels metadata entry), the function's ordinal in the file is blanked in local labels
(.LBB<n>_, .Lfunc_end<n>) and in the comments that quote them, and every SYM is reported as
`identical`, `DIFFERS`, `only at REV` or `only in the working tree`.  --rename OLD=NEW replaces
the mangled symbol OLD by NEW in REV's assembly first (a kernel that lost a template argument).
Exit status 1 if any kernel DIFFERS."""
import concurrent.futures
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_REL = os.path.join("point-cloud-cnn-segmentation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
JOBS = min(16, os.cpu_count() or 1)


def makefile_flags(csrc):
    """(sources, common flags, {source: extra flags}) as csrc/Makefile states them."""
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(rf"^{name} [:?]?= *(.*)$", mk, flags=re.M).group(1)
    flags = var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split()
    extra = {}
    for objs, val in re.findall(r"^([\w. ]+\.o): EXTRA := (.*)$", mk, flags=re.M):
        for o in objs.split():
            extra[o[:-2] + ".hip"] = val.split()
    return var("SRCS").split(), flags, extra


def device_asm(csrc, src, flags, extra, out):
    cmd = [HIPCC, *flags, *extra, "--cuda-device-only", "-S", "-o", out, src]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        return None, r.stderr
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", open(out).read()), r.stderr


def split_kernels(asm):
    """{symbol: its function, descriptor, resource summary and metadata entry}, ordinals blanked."""
    asm = re.sub(r"(\.L|\b)BB\d+_", r"\1BB_", re.sub(r"\.L(func_end|JTI)\d+", r".L\1", asm))
    asm = re.sub(r"[ \t]+;", " ;", asm)   # a comment's column moves with the width of the ordinal
    lines = asm.split("\n")
    meta = lines.index("\t.amdgpu_metadata") if "\t.amdgpu_metadata" in lines else len(lines)
    out, sym = {}, None
    for i, ln in enumerate(lines[:meta]):
        nxt = lines[i + 1] if i + 1 < meta else ""
        begin = re.search(r"; -- Begin function (\S+)", nxt if ln.startswith("\t.section\t.text") else ln)
        if begin and begin.group(1) != sym:
            sym = begin.group(1)
            out[sym] = []
        elif ln.startswith("\t.section\t.AMDGPU.gpr_maximums"):
            sym = None
        if sym:
            out[sym].append(ln)
    entry = []
    for ln in lines[meta:] + [""]:
        if not ln.startswith("    "):   # "  - " opens an amdhsa.kernels entry, a shallower line ends the list
            name = re.search(r"^    \.name: +(\S+)$", "\n".join(entry), flags=re.M)
            if name:
                out.setdefault(name.group(1), []).extend(entry)
            entry = []
        entry.append(ln)
    return {k: "\n".join(v) for k, v in out.items()}


def demangle(syms):
    """Readable names from binutils' c++filt where there is one, else the symbols themselves."""
    tool = shutil.which("c++filt")
    r = subprocess.run([tool, *syms], capture_output=True, text=True) if tool and syms else None
    names = r.stdout.splitlines() if r and r.returncode == 0 else []
    return dict(zip(syms, names)) if len(names) == len(syms) else {s: s for s in syms}


def report_kernels(name, a, b, rev, renames):
    """Print one line per kernel of a file; returns how many differ."""
    for old, new in renames:
        a = a.replace(old, new)
    ka, kb = split_kernels(a), split_kernels(b)
    syms = sorted(set(ka) | set(kb))
    nice = demangle(syms)
    bad = 0
    print(f"{name}:")
    for s in syms:
        if s not in ka or s not in kb:
            state = "only in the working tree" if s in kb else f"only at {rev}"
        elif ka[s] == kb[s]:
            state = "identical"
        else:
            state = "DIFFERS"
            bad += 1
        print(f"    {state:24s} {nice[s]}")
        if state == "DIFFERS":
            diff = difflib.unified_diff(ka[s].splitlines(), kb[s].splitlines(), rev, "working tree", n=1, lineterm="")
            for ln in list(diff)[:30]:
                print("        " + ln)
    return bad


def main(rev, only, kernels=False, renames=()):
    with tempfile.TemporaryDirectory() as tmp:
        old_root = os.path.join(tmp, "old")
        os.makedirs(old_root)
        tar = subprocess.run(["git", "-C", REPO, "archive", rev, "--", CSRC_REL, "include"], check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old_root], input=tar, check=True)
        sides = {"old": os.path.join(old_root, CSRC_REL), "new": os.path.join(REPO, CSRC_REL)}
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(JOBS) as pool:
            for side, csrc in sides.items():
                srcs, flags, extra = makefile_flags(csrc)
                for s in (s for s in srcs if not only or s in only):
                    out = os.path.join(tmp, f"{side}_{s}.s")
                    jobs[side, s] = pool.submit(device_asm, csrc, s, flags, extra.get(s, []), out)
        names = sorted({s for _, s in jobs})
        bad = 0
        for s in names:
            if ("old", s) not in jobs or ("new", s) not in jobs:
                print(f"{s:20s} only in {'the working tree' if ('new', s) in jobs else rev}")
                continue
            (a, aerr), (b, berr) = jobs["old", s].result(), jobs["new", s].result()
            if a is None or b is None:
                bad += 1
                print(f"{s:20s} DID NOT COMPILE\n{aerr if a is None else berr}")
            elif kernels:
                bad += 1 if report_kernels(s, a, b, rev, renames) else 0
            elif a == b:
                same_msgs = re.sub(r"\d+", "", aerr) == re.sub(r"\d+", "", berr)   # line numbers move
                print(f"{s:20s} identical" + ("" if same_msgs else "   (compiler messages differ)\n" + berr))
            else:
                bad += 1
                print(f"{s:20s} DIFFERS")
                diff = difflib.unified_diff(a.splitlines(), b.splitlines(), rev, "working tree", n=1, lineterm="")
                for i, ln in enumerate(diff):
                    if i >= 30:
                        break
                    print("    " + ln)
        what = "have no kernel that differs from" if kernels else "identical to"
        print(f"{len(names) - bad} of {len(names)} {what} {rev}")
        return 1 if bad else 0


if __name__ == "__main__":
    argv, renames = sys.argv[1:], []
    kernels = "--kernels" in argv
    while "--rename" in argv:
        i = argv.index("--rename")
        renames.append(tuple(argv[i + 1].split("=", 1)))
        del argv[i:i + 2]
    argv = [x for x in argv if x != "--kernels"]
    sys.exit(main(argv[0] if argv else "HEAD", argv[1:], kernels, renames))
