"""Instructions of ONE blend visit in a device assembly listing of raster_fwd.hip / raster_bwd.hip (developer tool): the count the
blend kernels' time follows (they are bound by vector-instruction issue).
usage: hipcc <build flags> --cuda-device-only -S syn3r_amd/csrc/raster_bwd.hip -o bwd.s ; python tools/visit_count.py bwd.s [more.s ...] [-v]
k_render_bwd<..>: from the label in front of the splat record's LDS reads to the LDS float atomic; k_render: the basic block(s) from
the label in front of the record's LDS reads to the loop's branch.  -v prints the instructions."""
import re
import sys

verbose = "-v" in sys.argv
for path in [a for a in sys.argv[1:] if a != "-v"]:
    text = open(path).read()
    for name in re.findall(r"\n(_Z\w*k_render\w*):", text):
        body = text.split("\n%s:" % name, 1)[1].split("\n.Lfunc_end", 1)[0].split("\n")
        if "k_render_bwd" in name:
            end = next(i for i, l in enumerate(body) if re.search(r"\tds_add(_rtn)?_f32", l))
            start = end
        else:
            start = next(i for i, l in enumerate(body) if "v_exp_f32" in l)
            end = next(i for i in range(start, len(body)) if re.search(r"\ts_c?branch", body[i]))
        while not re.search(r"\tds_read", body[start]):
            start -= 1
        while not body[start].startswith(".LBB"):
            start -= 1
        seg = [l.split(";")[0].strip() for l in body[start:end + 1] if l.startswith("\t") and not l.startswith("\t.")]
        seg = [l for l in seg if l]
        vec = [l for l in seg if l.startswith("v_")]
        kind = re.search(r"k_render(_bwdILb([01]))?", name)
        label = "k_render" if not kind.group(1) else "k_render_bwd<%s>" % ("true" if kind.group(2) == "1" else "false")
        print("%-28s %-22s vector %3d  of them packed %3d  all %3d" % (path, label, len(vec), len([l for l in vec if l.startswith("v_pk_")]), len(seg)))
        if verbose:
            print("\n".join("    " + l for l in seg))
