#!/usr/bin/env python3
"""Is the device code of every kernel source the same as at another revision?

    python tools/isa_identity.py REV

The gate of a refactor that must not change a kernel.  lkgd_amd/csrc and include/ of REV (git archive, no checkout) and of the
working tree are copied into a temporary directory each, every source in the Makefile's SRCS is compiled to device ISA there by
the WORKING TREE's Makefile (`make isa`: each object's own flags), the `__hip_cuid_<hash>` lines - a hash of the source text -
are dropped, and the two files of each source are compared as text.  Prints, per source, `identical` or the first kernel whose
body, descriptor or metadata differs, and the sha256 of each stripped file; exits 1 if any source differs.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("lkgd_amd", "csrc")
JOBS = 16


def strip_cuid(text):
    return "".join(l for l in text.splitlines(True) if "__hip_cuid_" not in l)


def _kernel_at(lines, i):
    """the kernel that line i belongs to: its function section, or its entry of the metadata list"""
    meta = max((k for k in range(i + 1) if lines[k].strip() == ".amdgpu_metadata"), default=-1)
    if meta >= 0:
        start = max((k for k in range(meta, i + 1) if lines[k].startswith("  - ")), default=meta)
        for l in lines[start + 1:]:
            if l.startswith("  - "):
                break
            m = re.match(r"    \.name:\s+(\S+)", l)
            if m:
                return m.group(1)
        return "(metadata)"
    for l in reversed(lines[:i + 1]):
        m = re.search(r"; -- Begin function (\S+)", l)
        if m:
            return m.group(1)
    return "(file header)"


def compare(a, b):
    """None if the two ISA texts are the same but for their __hip_cuid_ lines, else (kernel, line of a, line of b) at the
    first difference"""
    la, lb = strip_cuid(a).splitlines(), strip_cuid(b).splitlines()
    if la == lb:
        return None
    i = next((k for k, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
    at = lambda ls: ls[i].strip() if i < len(ls) else "(end of file)"
    return _kernel_at(la if i < len(la) else lb, i), at(la), at(lb)


def sources(makefile):
    return re.search(r"^SRCS\s*=\s*(.+)$", open(makefile).read(), re.M).group(1).split()


def emit_isa(tree, makefile, srcs):
    """device ISA of every source of `tree`, by the working tree's Makefile; {source: text}"""
    d = os.path.join(tree, CSRC)
    have = [s for s in srcs if os.path.exists(os.path.join(d, s))]
    r = subprocess.run(["make", "-C", d, "-f", makefile, "-j%d" % JOBS, "isa", "SRCS=" + " ".join(have)], capture_output=True, text=True)
    if r.returncode:
        sys.exit("make isa failed in %s:\n%s" % (d, r.stderr[-3000:]))
    return {s: open(os.path.join(d, s[:-4] + ".isa.s")).read() for s in have}


def main(rev):
    makefile = os.path.join(REPO, CSRC, "Makefile")
    srcs = sources(makefile)
    with tempfile.TemporaryDirectory() as tmp:
        old, new = os.path.join(tmp, "rev"), os.path.join(tmp, "tree")
        os.makedirs(old)
        ar = subprocess.run(["git", "-C", REPO, "archive", rev, CSRC, "include"], capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", old], input=ar.stdout, check=True)
        keep = shutil.ignore_patterns("*.o", "*.d", "*.s", "*.so")
        shutil.copytree(os.path.join(REPO, CSRC), os.path.join(new, CSRC), ignore=keep)
        shutil.copytree(os.path.join(REPO, "include"), os.path.join(new, "include"))
        isa_old, isa_new = emit_isa(old, makefile, srcs), emit_isa(new, makefile, srcs)
    sha = lambda t: hashlib.sha256(strip_cuid(t).encode()).hexdigest()
    rev_id = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", rev], capture_output=True, text=True).stdout.strip()
    print("device ISA (gfx950, __hip_cuid_ lines dropped): working tree against %s" % rev_id)
    differing = 0
    for s in srcs:
        if s not in isa_old:
            differing += 1
            print("%-24s absent at %s    sha256 %s" % (s, rev_id, sha(isa_new[s])))
            continue
        diff = compare(isa_old[s], isa_new[s])
        if diff is None:
            print("%-24s identical    sha256 %s" % (s, sha(isa_new[s])))
        else:
            differing += 1
            print("%-24s DIFFERS first in %s\n    %s: %s\n    tree: %s\n    sha256 %s (%s) %s (tree)"
                  % (s, diff[0], rev_id, diff[1], diff[2], sha(isa_old[s]), rev_id, sha(isa_new[s])))
    print("%d of %d sources identical" % (len(srcs) - differing, len(srcs)))
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
