"""Row tiling behind the drop-in API (SURVEY.md §8(b) `SetDevices(n)`, §8(e)).

* cpt_gather_rows: tiles rendered by separate contexts, gathered into one frame context, equal
  the monolithic render (accumulator and first-hit normals);
* PathTracer::SetDevices(n) through examples/headless_render.cpp: C5's 3840x2160 frame on 2 and
  8 contexts (all on device 0 here: a device may repeat) equals the single-context render bit
  for bit and the oracle on sampled rows; the DispatchRay display path over 2 contexts
  reproduces the golden BGRA8 frames.
"""
import os
import subprocess

import numpy as np
import pytest

from cpppathtracer_amd import CptError, Renderer, camera_get_copy, scenes, tiling

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _headless():
    from cpppathtracer_amd import build
    return build.build_examples()


@pytest.mark.parametrize("world", [2, 3])
def test_gather_rows_equals_monolithic(gpu, sky, world):
    objs = scenes.scene_s1000(n=300)
    W, H, spp, depth, seed = 80, 44, 3, 12, 21
    cam = camera_get_copy(scenes.camera_for(W, H))
    gpu.set_scene(objs)
    gpu.set_env(sky)
    gpu.set_frame(W, H)
    gpu.init_rng(seed)
    gpu.render(cam, spp, depth, aux=True, ordered=True, schedule="cost", sync=True)
    mono, (mono_n, mono_d) = gpu.read_accum(), gpu.read_aux()
    tiles = []
    try:
        for rank in range(world):
            t = Renderer(0)
            tiles.append(t)
            t.set_scene(objs)
            t.set_env(sky)
            t.set_frame(W, H, tiling.partition_rows(H, world, rank))
            t.init_rng(seed)
            t.render(cam, spp, depth, aux=True, ordered=True, schedule="cost")   # asynchronous
        with Renderer(0) as frame:
            frame.set_frame(W, H)
            for t in tiles:
                frame.gather_rows(t)
            acc, (nrm, dep) = frame.read_accum(), frame.read_aux()
            # a destination that does not hold the source's rows is refused
            with Renderer(0) as part:
                part.set_frame(W, H, tiling.partition_rows(H, world, 0))
                with pytest.raises(CptError):
                    part.gather_rows(tiles[1])
    finally:
        for t in tiles:
            t.close()
    np.testing.assert_array_equal(acc.view(np.uint32), mono.view(np.uint32))
    np.testing.assert_array_equal(nrm.view(np.uint32), mono_n.view(np.uint32))
    np.testing.assert_array_equal(dep, mono_d)


def _run(args, tmp_path, name):
    out = tmp_path / name
    r = subprocess.run([_headless(), *args, "--out", str(out)], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.fromfile(out, dtype=np.float32), r.stdout


def test_set_devices_c5_frame(oracle_mod, sky, tmp_path):
    """C5's frame (3840x2160, S1000, depth 16) at 2 spp: SetDevices(2) and SetDevices(8) equal
    the single-device image bit for bit, and the oracle on rows from every partition."""
    W, H, spp, depth = 3840, 2160, 2, 16
    base = ["--scene", "s1000", "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth),
            "--seed", "1234"]
    mono, _ = _run(base, tmp_path, "d1.bin")
    for n in (2, 8):
        got, stdout = _run(base + ["--devices", str(n)], tmp_path, f"d{n}.bin")
        assert f"on {n} device context(s)" in stdout, stdout
        np.testing.assert_array_equal(got.view(np.uint32), mono.view(np.uint32))
        os.remove(tmp_path / f"d{n}.bin")
    rows = np.array([0, 7, 8, 15, 16, 1079, 1080, 2151, 2159], dtype=np.int32)
    cam = oracle_mod.camera_get_copy(scenes.camera_for(W, H))
    rng = oracle_mod.init_rng(1234, W, rows, threads=8)
    acc, _, _, _ = oracle_mod.render(scenes.scene_s1000(), cam, sky, rows, spp, depth, rng, threads=8)
    want = (acc[:, :3] / acc[:, 3:4]).astype(np.float32)
    got_rows = mono.reshape(H, W, 3)[rows].reshape(-1, 3)
    np.testing.assert_array_equal(got_rows.view(np.uint32), want.view(np.uint32))


def test_set_devices_dispatch_pipeline(tmp_path):
    """InitPipeline + DispatchRay x3 over 2 row-tile contexts: each pass's tiles (with their
    first-hit normals) are gathered before the denoise + mix, so the BGRA8 frame is the golden
    single-device frame (path_tracer.cu:256-306)."""
    out = tmp_path / "frame.bin"
    r = subprocess.run([_headless(), "--scene", "s4", "--width", "64", "--height", "48", "--depth", "8",
                        "--dispatch", "3", "--bgra", str(out), "--devices", "2"], cwd=REPO, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    z = np.load(os.path.join(GOLDEN, "display_s4_64x48_3frames.npz"))
    np.testing.assert_array_equal(np.fromfile(out, dtype=np.uint8).reshape(48, 64, 4), z["bgra"])


# PathTracer over two row tiles on one device (SetDevices({0, 0}): a device may repeat) against a
# single-device tracer, in one small C++ program on the drop-in header: one sphere over a platform,
# depth 2, seed 7.  SceneBVH is process-global, so both tracers render the same scene; each has its
# own camera object (GetCopy advances the sample index).  argv[1] selects the case.
TILES_SRC = r"""
#include <cmath>
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

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

static void refusals() {
    Rig r(16, 16, true);
    PathTracer& t = r.tracer;
    const MotionalCamera from = *r.cam;
    expect(t.Render(1, false), "Render(1, false)");
    expect(!t.Reproject(from), "Reproject");
    expect_error(t, "Reproject: not available with SetDevices(n > 1), the row tiles own their accumulators");
    expect(!t.CaptureHistory(), "CaptureHistory");
    expect_error(t, "CaptureHistory: not available with SetDevices(n > 1), the row tiles own their accumulators");
    expect(!t.ReprojectTracked(), "ReprojectTracked");
    expect_error(t, "ReprojectTracked: not available with SetDevices(n > 1), the row tiles own their accumulators");
    expect(!t.FilterRadianceSpatial(), "FilterRadianceSpatial");
    expect_error(t, "FilterRadianceSpatial: not available with SetDevices(n > 1), the row tiles own their G-buffers");
    expect(t.Render(1, true), "Render(1, true) after the refusals");
    std::vector<float> rgb;
    expect(t.ReadRadiance(rgb), "ReadRadiance");
    expect(rgb.size() == 16 * 16 * 3, "ReadRadiance gives 16*16*3 floats");
    bool finite = true;
    for (float v : rgb) finite = finite && std::isfinite(v);
    expect(finite, "the radiance is finite");
}

static void topup() {
    std::vector<float> tiled, mono;
    {
        Rig r(16, 16, true);
        expect(r.tracer.Render(1, false), "tiles: Render(1, false)");
        expect(r.tracer.RenderToCount(3), "tiles: RenderToCount(3)");
        expect(r.tracer.ReadRadiance(tiled), "tiles: ReadRadiance");
    }
    {
        Rig r(16, 16, false);
        expect(r.tracer.Render(3, false), "one device: Render(3, false)");
        expect(r.tracer.ReadRadiance(mono), "one device: ReadRadiance");
    }
    expect(tiled.size() == 16 * 16 * 3, "16*16*3 floats");
    expect(same_bytes(tiled, mono), "RenderToCount(3) over tiles equals Render(3, false) on one device");
}

static void gbuffer() {
    const int W = 16, H = 24;
    std::vector<int32_t> id[2];
    std::vector<float> t[2], normal[2], albedo[2];
    for (int k = 0; k < 2; ++k) {
        Rig r(W, H, k == 0);
        expect(r.tracer.ReadGBuffer(id[k], t[k], normal[k], albedo[k]), k == 0 ? "tiles: ReadGBuffer" : "one device: ReadGBuffer");
    }
    expect(id[1].size() == (size_t)W * H && t[1].size() == (size_t)W * H, "id and t have W*H entries");
    expect(normal[1].size() == (size_t)3 * W * H && albedo[1].size() == (size_t)3 * W * H, "normal and albedo have 3*W*H");
    expect(same_bytes(id[0], id[1]), "id plane");
    expect(same_bytes(t[0], t[1]), "t plane");
    expect(same_bytes(normal[0], normal[1]), "normal plane");
    expect(same_bytes(albedo[0], albedo[1]), "albedo plane");
    // the frame tells its row blocks apart, so rows scattered to the wrong place would show
    if (t[1].size() == (size_t)W * H) {
        expect(std::memcmp(&t[1][0], &t[1][8 * W], 8 * W * sizeof(float)) != 0, "rows 0-7 differ from rows 8-15");
        expect(std::memcmp(&t[1][8 * W], &t[1][16 * W], 8 * W * sizeof(float)) != 0, "rows 8-15 differ from rows 16-23");
        expect(std::memcmp(&t[1][0], &t[1][16 * W], 8 * W * sizeof(float)) != 0, "rows 0-7 differ from rows 16-23");
    }
    bool sphere = false, platform = false;
    for (int32_t i : id[1]) { sphere = sphere || i == 1; platform = platform || i == 0; }
    expect(sphere && platform, "the frame sees the sphere and the platform");
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
    if (what == "refusals") refusals();
    else if (what == "topup") topup();
    else if (what == "gbuffer") gbuffer();
    else expect(false, "unknown case");
    printf("bad %d\n", bad);
    return bad != 0;
}
"""


@pytest.fixture(scope="module")
def tiles_exe(tmp_path_factory):
    from cpppathtracer_amd import _lib
    d = tmp_path_factory.mktemp("tiles_api")
    src, exe = d / "tiles.cpp", d / "tiles"
    src.write_text(TILES_SRC)
    lib = _lib.lib_path()
    assert os.path.exists(lib), lib
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I", os.path.join(REPO, "include"), "-o", str(exe),
                    str(src), lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return str(exe)


def _tiles_case(exe, case):
    r = subprocess.run([exe, case], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad 0" in r.stdout, r.stdout + r.stderr


def test_row_tiles_refuse_single_accumulator_calls(tiles_exe):
    """With two row tiles Reproject, CaptureHistory, ReprojectTracked and FilterRadianceSpatial
    return false with their exact messages, and the tracer renders on afterwards."""
    _tiles_case(tiles_exe, "refusals")


def test_row_tiles_render_to_count_equals_single_device_render(tiles_exe):
    """Render(1, false) + RenderToCount(3) over two row tiles is Render(3, false) on one device,
    byte for byte through ReadRadiance (the contract of RenderToCount, on the tiled launch and
    gather)."""
    _tiles_case(tiles_exe, "topup")


def test_row_tiles_read_gbuffer_equals_single_device(tiles_exe):
    """ReadGBuffer of a 16x24 frame over two row tiles (rows 0-7 and 16-23 on the first, 8-15 on
    the second) equals the single-device G-buffer in all four planes, byte for byte."""
    _tiles_case(tiles_exe, "gbuffer")
