#!/usr/bin/env python3
"""Compare the kernels of the UNITS' device code between a commit and the working tree, kernel
by kernel: the instruction stream with its local label numbers normalised, and the register, spill,
scratch and LDS figures of the code object's metadata.

    tools/isa_compare.py [REV] > profiles/rNN/refactor_isa.log      (REV: the parent, default HEAD)

Both sides are compiled with the flags of cpppathtracer_amd/build.py plus --cuda-device-only -S.
The log's header names both sides, the compiler and the flags.  Exit status 1 if a kernel's stream
or figures differ, or it is missing on one side.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cpppathtracer_amd import build as _build   # noqa: E402

UNITS = ["cpt_megakernel", "cpt_wavefront", "cpt_query", "cpt_display", "cpt_schedule"]
FLAGS = [f for f in _build.HIPCC_FLAGS if f != "-shared"] + ["--cuda-device-only", "-S"]
META = [".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size"]
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def sh(*cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def compile_units(root, out):
    def one(u):
        subprocess.run([_build._hipcc(), *FLAGS, "-Wno-unused-command-line-argument", "-I", os.path.join(root, "include"),
                        "-o", os.path.join(out, u + ".s"), os.path.join(root, "cpppathtracer_amd", "csrc", u + ".hip")],
                       check=True)
    with ThreadPoolExecutor(len(UNITS)) as ex:
        list(ex.map(one, UNITS))


def demangle(names):
    try:
        out = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    """{kernel symbol: (normalised instruction lines, {metadata key: value})}"""
    lines = open(path).read().splitlines()
    kernels = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    streams = {}
    i = 0
    while i < len(lines):
        head = lines[i].split(";")[0].rstrip()
        name = head[:-1] if head.endswith(":") else None
        if name in kernels and name not in streams:
            body, labels = [], {}
            i += 1
            while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
                code = lines[i].split(";")[0].rstrip()
                i += 1
                if not code or (code.lstrip().startswith(".") and not code.endswith(":")):
                    continue   # comments, blank lines, assembler directives
                code = LABEL.sub(lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), code)
                body.append(" ".join(code.split()))
            streams[name] = body
        i += 1
    # amdhsa.kernels: one "  - .key: value" entry per kernel, its other keys indented by four
    meta, cur = {}, None
    for l in lines[lines.index("amdhsa.kernels:") + 1:] if "amdhsa.kernels:" in lines else []:
        if l.startswith("  - "):
            cur = {}
        m = re.match(r"(?:  - |    )(\.[a-z_]+):\s*(\S+)$", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                meta[m.group(2)] = cur
    return {k: (streams.get(k, []), meta.get(k, {})) for k in kernels}


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    parent = sh("git", "-C", REPO, "rev-parse", rev).strip()
    head = sh("git", "-C", REPO, "rev-parse", "HEAD").strip()
    dirty = bool(sh("git", "-C", REPO, "status", "--porcelain", "--", "cpppathtracer_amd/csrc", "include").strip())
    print("# parent: %s" % parent)
    print("# new:    %s%s" % (head, " + the working tree's uncommitted changes" if dirty else ""))
    print("# %s" % " | ".join(sh(_build._hipcc(), "--version").splitlines()[:2]))
    print("# flags:  %s" % " ".join(FLAGS))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        a_dir, b_dir, src = (os.path.join(tmp, d) for d in ("parent", "new", "src"))
        for d in (a_dir, b_dir, src):
            os.mkdir(d)
        tar = subprocess.run(["git", "-C", REPO, "archive", parent, "cpppathtracer_amd/csrc", "include"], check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", src], input=tar, check=True)
        compile_units(src, a_dir)
        compile_units(REPO, b_dir)
        print("# kernel | parent: instructions, " + ", ".join(k[1:] for k in META) +
              " | new: the same | identical (else: lines of the streams' unified diff)")
        for unit in UNITS:
            a, b = parse(os.path.join(a_dir, unit + ".s")), parse(os.path.join(b_dir, unit + ".s"))
            names = demangle(sorted(set(a) | set(b)))
            print("## " + unit)
            for k in sorted(names, key=names.get):
                sa, ma = a.get(k, ([], {}))
                sb, mb = b.get(k, ([], {}))
                same = k in a and k in b and sa == sb and all(ma.get(m) == mb.get(m) for m in META)
                bad += not same
                fig = lambda s, m: "%d %s" % (len(s), " ".join(m.get(x, "-") for x in META))
                verdict = "yes" if same else "NO (%d)" % sum(
                    1 for l in difflib.unified_diff(sa, sb, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
                print("%s | %s | %s | %s" % (names[k], fig(sa, ma), fig(sb, mb), verdict))
    print("# %s" % ("all identical" if not bad else "%d kernels differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
