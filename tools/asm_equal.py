"""Is the gfx950 device code of every csrc/*.hip the same as at a git revision?  (no GPU needed)

    python tools/asm_equal.py [REV [FILE.hip ...]]        (default: HEAD, every file)

Compiles every source of csrc/Makefile's SRCS to device assembly (the Makefile's CXXFLAGS and
per-file EXTRA flags plus --cuda-device-only -S), once as committed at REV (sources and headers
extracted into a temporary tree) and once from the working tree, blanks the __hip_cuid_<hash>
symbol (a hash of the source text) and prints per file `identical` or the first differing lines.
The assembly carries the register, LDS, spill and scratch counts of every kernel, so `identical`
for every file is "same machine code": the check for a refactor that must not change any.
Exit status 1 if any file differs."""
import concurrent.futures
import difflib
import os
import re
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


def main(rev, only):
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
        print(f"{len(names) - bad} of {len(names)} identical to {rev}")
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "HEAD", sys.argv[2:]))
