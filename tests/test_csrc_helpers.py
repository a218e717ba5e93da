"""csrc/kernel_prims.h holds the one definition of the shared device primitives (LDS-DMA
statements, counted waits, barriers, XCD remap, fragment reads): no kernel file grows a copy of
its own again.  A source-text check: no compiler, no GPU."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "point-cloud-cnn-segmentation_amd", "csrc")
# a function defined at namespace scope the way common.h and kernel_prims.h define theirs
# (members of a struct are indented and are not meant)
DEF = re.compile(r"^(?:template <[^>]*> )?PCS_DEV [\w:<>&*]+ \*?(\w+)\(", flags=re.M)
# a per-kernel overload with another parameter list that shares a header name on purpose
LOCAL_OVERLOADS = {("fused_c5.hip", "lds_vec8")}   # (p, half_bytes, v): the split coefficient layout


def test_no_kernel_file_redefines_a_shared_primitive():
    shared = set(DEF.findall(open(os.path.join(CSRC, "kernel_prims.h")).read()))
    assert {"xcd_remap", "wait_vm", "barrier_lds", "m0_save", "m0_restore", "glds16", "glds16o", "glds4o",
            "glds16_keep_m0", "tr_frag2"} <= shared, shared   # the pattern still reads the header
    again = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        name = os.path.basename(path)
        again += [(name, f) for f in DEF.findall(open(path).read())
                  if f in shared and (name, f) not in LOCAL_OVERLOADS]
    assert not again, again
