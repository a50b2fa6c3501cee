"""Every fail(...) message of the C ABI's implementation files is in the recorded contract
(tests/golden/capi_contract.json, tests/test_gpu_capi_contract.py), or is exempt below for one of
the reasons that keep it out of a GPU test's reach.  The format strings are read out of
cpt_capi*.cpp and out of cpt_context.hpp, where the checks several files share live; each becomes a
pattern with every % conversion a wildcard."""
import glob
import json
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "cpppathtracer_amd", "csrc")
FIXTURE = os.path.join(REPO, "tests", "golden", "capi_contract.json")

HIP = "needs a failing HIP call or allocation"
DEVICE_WORD = "needs a device-side error word"
HUGE_FRAME = "needs a frame beyond 65,535 pixels per axis or UINT32_MAX/64 tiles"
TIMELINE = "needs a CPT_TIMELINE build"
REGISTER = "cpt_host_register / cpt_host_unregister failures"

# format string -> reason
EXEMPT = {
    "device error 0x%x:%s%s%s": DEVICE_WORD,
    "%s: device error 0x%x": DEVICE_WORD,
    "%s: %u of %u tiles kept": DEVICE_WORD + " (unreachable otherwise: the compaction keeps a subset of the list)",
    "cpt_debug_read_tile_order: %u of %zu tiles active":
        DEVICE_WORD + " (unreachable otherwise: the plan counts tiles of the frame)",
    "cpt_create: no HIP device visible": HIP + " (hipGetDeviceCount fails or finds none)",
    "cpt_create: host allocation failed": HIP,
    "cpt_create: %s": HIP,
    "motion table: host allocation failed": HIP,
    "cpt_history_capture: host allocation failed": HIP,
    "the captured history holds %zu objects, the scene %zu":
        "unreachable: cpt_set_scene, the only call that changes the object count, drops the captured history",
    "cpt_gbuffer: frame of %zu 8x8 tiles (max %u)": HUGE_FRAME,
    "%s: frame of %zu 8x8 tiles (max %u)": HUGE_FRAME,
    "cpt_debug_timeline: %s": TIMELINE + " (and a failing HIP call in it)",
    "cpt_host_register: %s": REGISTER,
    "cpt_host_unregister: %s": REGISTER,
}

# fail(<context>, <status>, "format" ["continued" ...]
FAIL = re.compile(r'\bfail\(\s*[^,()]+,\s*CPT_ERR_[A-Z_]+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)')
CONVERSION = re.compile(r"%[-+ #0]*\d*(?:\.\d+)?(?:hh|h|ll|l|z|j|t)?[diouxXeEfgGcsp]")


def fail_formats():
    """(file, format string) of every fail(...) call with a literal format."""
    out = []
    for path in sorted(glob.glob(os.path.join(CSRC, "cpt_capi*.cpp"))) + [os.path.join(CSRC, "cpt_context.hpp")]:
        with open(path) as fh:
            src = fh.read()
        for m in FAIL.finditer(src):
            fmt = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1)))
            out.append((os.path.basename(path), fmt))
    return out


def pattern_of(fmt):
    parts = CONVERSION.split(fmt.replace("%%", "%"))
    return re.compile(".*".join(re.escape(p) for p in parts), re.DOTALL)


def test_every_fail_site_is_found():
    # the sites as `grep -c 'fail('` counts them, less the definition, its declaration's neighbours
    # in comments and the macro: a format the pattern above cannot read would go unchecked
    formats = fail_formats()
    sites = 0
    for path in sorted(glob.glob(os.path.join(CSRC, "cpt_capi*.cpp"))) + [os.path.join(CSRC, "cpt_context.hpp")]:
        with open(path) as fh:
            for line in fh:
                code = line.split("//")[0]
                sites += len(re.findall(r"\bfail\(", code)) - len(re.findall(r"\bint fail\(", code))
    assert len(formats) == sites and sites >= 100


def test_every_message_is_recorded_or_exempt():
    with open(FIXTURE) as fh:
        texts = sorted({step[4] for step in json.load(fh) if step[3] != 0})
    formats = fail_formats()
    missing = []
    for name, fmt in formats:
        if fmt in EXEMPT:
            continue
        if fmt == "%s":   # last_span_ms passes the caller's whole text: the callers' literals are checked below
            continue
        rx = pattern_of(fmt)
        if not any(rx.fullmatch(t) for t in texts):
            missing.append((name, fmt))
    assert not missing, f"fail(...) messages neither in {os.path.relpath(FIXTURE, REPO)} nor exempt: {missing}"
    stale = sorted(set(EXEMPT) - {fmt for _, fmt in formats})
    assert not stale, f"exemptions without a fail(...) site: {stale}"


def test_every_nothing_yet_text_is_recorded():
    """The texts last_span_ms reports through its "%s": each cpt_last_*_ms entry's own literal."""
    with open(FIXTURE) as fh:
        texts = {step[4] for step in json.load(fh)}
    found = []
    for path in sorted(glob.glob(os.path.join(CSRC, "cpt_capi*.cpp"))):
        with open(path) as fh:
            src = fh.read()
        for m in re.finditer(r'last_span_ms\(c,\s*&cpt_ctx::\w+,\s*&?\w+,\s*"((?:[^"\\]|\\.)*)"\)', src):
            found.append(m.group(1))
    assert len(found) == 7
    assert not [t for t in found if t not in texts]
