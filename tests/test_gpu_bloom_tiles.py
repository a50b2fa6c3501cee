"""PathTracer's bloom over two row tiles, in the manner of
tests/test_gpu_antialias_tiles.py: a small C++ program on the drop-in header with SetDevices({0, 0}).
BuildBloom and PresentBloom each return false with their exact messages, write nothing and leave the
tracer rendering; on one device the same calls succeed, and PresentBloom before any BuildBloom
reports the missing pyramid."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cpppathtracer/path_tracer.h"

static int bad = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { printf("FAILED: %s\n", what); ++bad; }
}
static void expect_error(const PathTracer& t, const std::string& want) {
    if (t.LastError() != want) { printf("FAILED: LastError \"%s\", expected \"%s\"\n", t.LastError().c_str(), want.c_str()); ++bad; }
}

static Object* make_object(PrimitiveType::Enum type, float3 kd) {
    Object* o = new Object();
    std::memset(o, 0, sizeof(Object));
    o->type_ = type;
    o->material_.type_ = MaterialType::Diffuse;
    o->material_.kd_ = kd;
    return o;
}

struct Rig {
    PathTracer tracer;
    std::shared_ptr<MotionalCamera> cam;
    Rig(int w, int h, bool tiled)
        : cam(new MotionalCamera(w, h, make_float3(130.f, 103.f, 130.f), make_float3(0.f, 0.f, 0.f))) {
        tracer.SetCamera(cam);
        tracer.SetSeed(7);
        expect(tracer.SetMaxRecursionDepth(2), "SetMaxRecursionDepth");
        if (tiled) expect(tracer.SetDevices(std::vector<int>{0, 0}), "SetDevices({0, 0})");
        expect(tracer.DeviceCount() == (tiled ? 2 : 1), "DeviceCount");
    }
};

static void tiles() {
    Rig r(16, 16, true);
    PathTracer& t = r.tracer;
    expect(t.Render(1, false), "Render(1, false)");
    std::vector<uint8_t> bgra(5, 77);
    // no BuildBloom came before: the refusal is PresentBloom's own
    expect(!t.PresentBloom(bgra), "PresentBloom over two tiles");
    expect_error(t, "PresentBloom: not available with SetDevices(n > 1), the row tiles own their accumulators");
    expect(bgra.size() == 5 && bgra[0] == 77 && bgra[4] == 77, "a refused PresentBloom leaves the caller's vector alone");
    expect(!t.BuildBloom(), "BuildBloom over two tiles");
    expect_error(t, "BuildBloom: not available with SetDevices(n > 1), the row tiles own their accumulators");
    expect(!t.PresentBloom(bgra, CPT_TONE_CLAMP, false), "PresentBloom again");
    expect_error(t, "PresentBloom: not available with SetDevices(n > 1), the row tiles own their accumulators");
    expect(bgra.size() == 5 && bgra[0] == 77, "and again nothing is written");
    expect(t.Render(1, true), "Render(1, true) after the refusals");
    std::vector<float> rgb;
    expect(t.ReadRadiance(rgb) && rgb.size() == 16 * 16 * 3, "ReadRadiance");
}

static void single() {
    Rig r(16, 16, false);
    PathTracer& t = r.tracer;
    expect(t.Render(2, false), "Render(2, false)");
    std::vector<uint8_t> plain, glow, none;
    expect(!t.PresentBloom(glow), "PresentBloom before any BuildBloom");
    expect(t.LastError().find("cpt_present_bloom: no pyramid (cpt_bloom first)") != std::string::npos, "the missing pyramid is named");
    expect(glow.empty(), "and nothing is written");
    expect(!t.BuildBloom(false, 1.0f, 9), "BuildBloom(levels 9)");
    expect(t.LastError().find("cpt_bloom: source 0, threshold 1 (finite, >= 0), levels 9 (1..8)") != std::string::npos, "the bad level count is named");
    expect(t.BuildBloom(false, 0.05f, 4), "BuildBloom");
    expect(!t.PresentBloom(glow, CPT_TONE_ACES, true, false, 4.0f, -1.0f), "PresentBloom(intensity -1)");
    expect(glow.empty(), "a refused PresentBloom writes nothing");
    expect(t.PresentBloom(glow, CPT_TONE_ACES, true, false, 4.0f, 1.0f), "PresentBloom");
    expect(t.PresentBloom(none, CPT_TONE_ACES, true, false, 4.0f, 0.0f), "PresentBloom(intensity 0)");
    expect(t.Present(plain), "Present");
    expect(glow.size() == 16 * 16 * 4 && plain.size() == glow.size(), "16*16*4 bytes each");
    expect(none == plain, "intensity 0 gives Present's bytes");
    // the lit floor is above the threshold: its light reaches the neighbouring pixels
    expect(glow != plain, "the bloomed frame differs from the plain one");
    bool opaque = true;
    for (size_t i = 3; i < glow.size(); i += 4) opaque = opaque && glow[i] == 255;
    expect(opaque, "alpha 255");
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    Object* floor = make_object(PrimitiveType::Platform, make_float3(0.95f, 0.95f, 0.95f));
    floor->y_pos_ = 0.f;
    Object* ball = make_object(PrimitiveType::Sphere, make_float3(0.8f, 0.3f, 0.3f));
    ball->center_ = make_float3(0.f, 15.f, 0.f);
    ball->radius_ = 15.f;
    SceneBVH::AddObject(floor);
    SceneBVH::AddObject(ball);
    if (what == "tiles") tiles();
    else if (what == "single") single();
    else expect(false, "unknown case");
    printf("bad %d\n", bad);
    return bad != 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cpppathtracer_amd import _lib
    d = tmp_path_factory.mktemp("bloom_api")
    src, out = d / "bloom_api.cpp", d / "bloom_api"
    src.write_text(SRC)
    lib = _lib.lib_path()
    assert os.path.exists(lib), lib
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I", os.path.join(REPO, "include"), "-o", str(out),
                    str(src), lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return str(out)


def _case(exe, case):
    r = subprocess.run([exe, case], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad 0" in r.stdout, r.stdout + r.stderr


def test_row_tiles_refuse_bloom(exe):
    """With two row tiles BuildBloom and PresentBloom (with no BuildBloom before it) return false
    with their exact messages, write nothing, and the tracer renders on afterwards."""
    _case(exe, "tiles")


def test_one_device_builds_and_presents(exe):
    """On one device: PresentBloom before any BuildBloom names the missing pyramid, a bad level count
    and a bad intensity are refused, then both calls succeed; intensity 0 gives Present's bytes and
    intensity 1 does not."""
    _case(exe, "single")
