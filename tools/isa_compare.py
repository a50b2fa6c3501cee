#!/usr/bin/env python3
"""Compare the kernels of the UNITS' device code between a commit and the working tree, kernel
by kernel: the instruction stream with its local label numbers normalised, and the register, spill,
scratch and LDS figures of the code object's metadata.

    tools/isa_compare.py [REV] [--rename 'OLD=NEW' ...] > profiles/rNN/refactor_isa.log
                                                                    (REV: the parent, default HEAD)

--rename compares the parent's kernel OLD with the new side's kernel NEW (demangled names, as the log
prints them): a kernel template that gained a parameter keeps its instantiations under new names.

Both sides are compiled with the flags of cpppathtracer_amd/build.py plus --cuda-device-only -S.
The log's header names both sides, with the git tree ids of their sources (`git rev-parse
COMMIT:cpppathtracer_amd/csrc` gives the same id for the commit a side belongs to), the compiler and
the flags.  Exit status 1 if a kernel's stream
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

UNITS = ["cpt_megakernel", "cpt_wavefront", "cpt_query", "cpt_display", "cpt_schedule", "cpt_reproject", "cpt_adaptive",
         "cpt_filter", "cpt_topup", "cpt_kernels", "cpt_selftest", "cpt_present", "cpt_antialias"]
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


SOURCE_DIRS = ["cpppathtracer_amd/csrc", "include"]


def tree_ids(rev=None):
    """The git tree ids of SOURCE_DIRS at `rev`, or (None) of the working tree's files as a commit of
    them would record them: what `git rev-parse COMMIT:DIR` prints for that commit, so a log made
    before the commit can be tied to it."""
    if rev:
        return [sh("git", "-C", REPO, "rev-parse", "%s:%s" % (rev, d)).strip() for d in SOURCE_DIRS]
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, GIT_INDEX_FILE=os.path.join(tmp, "index"))
        sh("git", "-C", REPO, "read-tree", "HEAD", env=env)
        sh("git", "-C", REPO, "add", "-A", "--", *SOURCE_DIRS, env=env)
        return [sh("git", "-C", REPO, "write-tree", "--prefix=%s/" % d, env=env).strip() for d in SOURCE_DIRS]


def main():
    args = sys.argv[1:]
    renames = {}
    while "--rename" in args:
        i = args.index("--rename")
        old, new = args[i + 1].split("=", 1)
        renames[new.strip()] = old.strip()
        del args[i:i + 2]
    rev = args[0] if args else "HEAD"
    parent = sh("git", "-C", REPO, "rev-parse", rev).strip()
    head = sh("git", "-C", REPO, "rev-parse", "HEAD").strip()
    dirty = bool(sh("git", "-C", REPO, "status", "--porcelain", "--", "cpppathtracer_amd/csrc", "include").strip())
    sources = lambda ids: ", ".join("%s %s" % (d, i) for d, i in zip(SOURCE_DIRS, ids))
    print("# parent: %s (trees: %s)" % (parent, sources(tree_ids(parent))))
    print("# new:    %s (trees: %s)" % ("the working tree, not yet a commit" if dirty else head, sources(tree_ids())))
    print("# %s" % " | ".join(sh(_build._hipcc(), "--version").splitlines()[:2]))
    print("# flags:  %s" % " ".join(FLAGS))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        a_dir, b_dir, src = (os.path.join(tmp, d) for d in ("parent", "new", "src"))
        for d in (a_dir, b_dir, src):
            os.mkdir(d)
        tar = subprocess.run(["git", "-C", REPO, "archive", parent, *SOURCE_DIRS], check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", src], input=tar, check=True)
        compile_units(src, a_dir)
        compile_units(REPO, b_dir)
        print("# kernel | parent: instructions, " + ", ".join(k[1:] for k in META) +
              " | new: the same | identical (else: lines of the streams' unified diff)")
        for unit in UNITS:
            a, b = parse(os.path.join(a_dir, unit + ".s")), parse(os.path.join(b_dir, unit + ".s"))
            names = demangle(sorted(set(a) | set(b)))
            # a renamed kernel: the parent's entry moves under the new symbol, its own row goes
            symbol = {v: k for k, v in names.items()}
            for new, old in renames.items():
                if new in symbol and old in symbol and symbol[old] in a:
                    a[symbol[new]] = a.pop(symbol[old])
                    names[symbol[new]] = "%s (parent: %s)" % (new, old)
                    if symbol[old] not in b:
                        del names[symbol[old]]
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
