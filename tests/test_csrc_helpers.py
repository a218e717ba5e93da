"""The shared headers of csrc hold the one definition of what several kernel files use:
kernel_prims.h the device primitives of the hand-scheduled kernels (LDS-DMA statements, counted
waits, barriers, XCD remap, fragment reads), row_piece.h the row-piece helpers of the
bandwidth-bound row kernels, voxel_geom.h the voxel box and id.  No kernel file grows a copy of
its own again.  A source-text check: no compiler, no GPU."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "point-cloud-cnn-segmentation_amd", "csrc")
HEADERS = ("kernel_prims.h", "row_piece.h", "voxel_geom.h")
# a function defined at namespace scope the way common.h and the shared headers define theirs
# (members of a struct are indented and are not meant; a template line may stand above)
DEF = re.compile(r"^(?:template <[^>]*> )?PCS_DEV [\w:<>&*]+ \*?(\w+)\(", flags=re.M)
# a struct defined at namespace scope (a template line may stand above)
STRUCT = re.compile(r"^struct (\w+) \{", flags=re.M)
# a per-kernel overload with another parameter list that shares a header name on purpose
LOCAL_OVERLOADS = {("fused_c5.hip", "lds_vec8")}   # (p, half_bytes, v): the split coefficient layout


def test_no_kernel_file_redefines_a_shared_primitive():
    text = "".join(open(os.path.join(CSRC, h)).read() for h in HEADERS)
    shared, structs = set(DEF.findall(text)), set(STRUCT.findall(text))
    # the patterns still read the headers
    assert {"xcd_remap", "wait_vm", "barrier_lds", "m0_save", "m0_restore", "glds16", "glds16o", "glds4o",
            "glds16_keep_m0", "tr_frag2", "raw_load", "raw_unpack", "raw_fma", "store_piece", "lane_slot",
            "lane_slot_wide", "voxel_of"} <= shared, shared
    assert {"Raw", "Piece", "Box"} <= structs, structs
    again = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        name, src = os.path.basename(path), open(path).read()
        again += [(name, f) for f in DEF.findall(src) if f in shared and (name, f) not in LOCAL_OVERLOADS]
        again += [(name, "struct " + s) for s in STRUCT.findall(src) if s in structs]
    assert not again, again
