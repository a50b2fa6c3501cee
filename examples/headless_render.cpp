// headless_render.cpp — the reference app's scene setup (cppSrc/video_renderer.cpp:32-120)
// written against the drop-in C++ API, with the Win32 window replaced by file output.
//
//   cpt_headless [--scene s3|s4|s1000] [--width W] [--height H] [--spp N] [--depth D] [--seed S]
//                [--out radiance.bin] [--dispatch K --bgra frame.bin] [--pfm image.pfm]
//                [--texture file.ppm|file.cptex] [--dump-scene objects.bin] [--devices N]
//                [--objects N] [--animate K [--animate-step X]] [--pick X,Y] [--orbit N [--reproject]]
//                [--orbit N [--animate K] --display-reproject on|off|edits --bgra frame.bin]
//                [--animate K --reproject] [--fill T] [--filter-spatial [LEVELS] [--look-aside]]
//                [--present clamp|reinhard|aces [--exposure auto|X] [--linear] [--aa 2|4] --bgra frame.bin]
//                [--present CURVE --bloom THRESHOLD[,LEVELS[,INTENSITY]] --bgra frame.bin]
//
// --present CURVE (with plain --spp, and with --orbit N --reproject [--fill T] [--filter-spatial]; not
// with --display-reproject or --dispatch, whose loop has its own 8-bit output): the last frame, the
// filtered one with --filter-spatial, is presented through the exposure, the tone curve and the sRGB
// transfer (PathTracer::Present; --linear: the reference's 255.99 * linear bytes) and
// --bgra gets the BGRA8 frame.  --exposure auto meters the frame first (PathTracer::MeterExposure: the
// median luminance to 0.18), --exposure X sets it; without either it is 1.  --aa S (2 or 4; only with
// --present): S x S first-hit rays inside every edge pixel and the coverage-weighted presentation
// (PathTracer::ResolveCoverage, PresentAntialiased).  --bloom THRESHOLD[,LEVELS[,INTENSITY]]
// (only with --present, not with --aa; 6 levels and intensity 0.25 by default): the exposed light
// above THRESHOLD spread over LEVELS halvings and added in front of the tone curve
// (PathTracer::BuildBloom, PresentBloom).
//
// --filter-spatial [LEVELS] (without --adaptive: with plain --spp, and with --orbit N --reproject
// [--fill T]): the last frame is filtered without moments, its variance estimated from each pixel's
// neighbourhood and the levels guided by the G-buffer (PathTracer::FilterRadianceSpatial, DESIGN.md
// §25; 3 levels by default), and --pfm gets the filtered image.  With --look-aside the camera then
// turns one degree, PathTracer::ReadGBuffer is read there (an editor's overlay at the new view: the
// context's G-buffer is now that camera's) and the frame is filtered again: the radiance still
// belongs to the camera it was rendered with, so the second result, which --pfm gets, is the first's.
//
// --fill T (with --orbit N --reproject, and with --animate K --reproject): each frame after the
// first is topped up to T passes per pixel (PathTracer::RenderToCount) instead of
// given --spp uniform passes: the passes go to the pixels the reprojection left short.
//
// --orbit N --display-reproject on|off drives the DispatchRay pipeline through the same orbit: --spp
// passes at each of the N cameras (each waited for), every move followed by MotionalCamera::Refresh
// as the reference's viewer does, and writes the last BGRA8 frame to --bgra.  `on` sets
// PathTracer::SetDisplayReprojection, which carries the running mean to each new camera; `off` is
// the reference's loop, a fresh mean after every move.  With --animate K the loop goes on for K
// more frames of --spp passes at the last camera, every tenth object moved before each (no
// Refresh); `edits` sets SetDisplayReprojection's through_edits, which carries the mean through
// those edits as well, where `on` keeps the stale mean and `off` the reference's.
//
// --orbit N renders N frames of --spp passes each into one accumulator while the camera turns about
// the vertical axis through its look-at point, one degree per frame.  Without --reproject the
// frames are simply added (the image smears); with it PathTracer::Reproject carries the history to
// each new camera first.  --out / --pfm then hold the last frame.
//
// --pick X,Y prints the object (AddObject index, -1 = sky) under pixel (X, Y) of the image and its
// distance (PathTracer::Pick: one centre ray, no render), then exits.
//
// --devices N row-tiles the image over N contexts (PathTracer::SetDevices: device i % visible
// devices, so N > the GPU count puts several tiles on one GPU) and gathers each pass's tiles
// into one frame; the image is the single-device image, bit for bit.  So are --adaptive and
// --filter with it: the tiles' rounds run side by side and their moments are gathered too.
//
// --dump-scene writes the objects as SceneBVH::BuildBVH copied them (cpt_object records, the
// C-ABI layout) and exits without rendering (no GPU needed).
//
// --texture makes the floor, the Glass and the Metal sphere of s4 textured materials
// (Material::have_tex_/tex_, material.h:21-25) sampling that file (AddTexByFile defaults).
//
// --animate K renders K more frames after the first (spp each, not accumulated; the RNG streams
// continue), moving every 10th object (indices 1, 11, 21, ...) by +0.75 (--animate-step) in x before each one
// through SceneBVH::UpdateObject (a device refit of both trees), and prints each frame's time.
// --out then holds the last frame.  With --reproject the K frames are added to the first frame's
// accumulator instead, PathTracer::CaptureHistory before the first edit and ReprojectTracked after
// each carrying the history to where the objects moved.
// --out writes the raw accumulator mean as float32 rgb (row-major); --dispatch runs K passes
// through the asynchronous DispatchRay pipeline (1 spp + denoise + mix per pass, callback on
// the render thread) and writes the last BGRA8 frame to --bgra.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "cpppathtracer/path_tracer.h"

namespace {

std::vector<Object*> g_objects;   // AddObject order (--animate edits them)

void add(PathTracer& tracer, Object* o) {
    g_objects.push_back(o);
    tracer.AddObject(o);
}

Object* make_sphere(const Material& m, float3 c, float r) {
    Object* o = new Object();
    std::memset(o, 0, sizeof(Object));
    o->type_ = PrimitiveType::Sphere;
    o->material_ = m;
    o->center_ = c;
    o->radius_ = r;
    return o;
}

Material make_material(MaterialType::Enum t, float3 kd, float ior = 0.f, float smooth = 0.f, float refl = 0.f) {
    Material m;
    std::memset(&m, 0, sizeof(Material));
    m.type_ = t;
    m.have_tex_ = false;
    m.kd_ = kd;
    m.refractive_index_ = ior;
    m.smoothness_ = smooth;
    m.reflectivity_ = refl;
    return m;
}

Object* make_object(PrimitiveType::Enum t, const Material& m, float3 c, float r, float h) {
    Object* o = make_sphere(m, c, r);
    o->type_ = t;
    o->height_ = h;
    return o;
}

// MSVC rand() (RAND_MAX 32767) and the reference's random() (ray_tracing_math.hpp:30-37),
// seeded with a constant instead of time(0) so every run builds the same scene.
struct MsvcRand {
    uint32_t x;
    int rand() {
        x = x * 214013u + 2531011u;
        return (int)((x >> 16) & 0x7FFF);
    }
    float random() { return static_cast<float>(rand()) / static_cast<float>(32767); }
    float3 random3() {
        float a = random(), b = random(), c = random();
        return make_float3(a, b, c);
    }
};

// S1000: the floor + n random spheres / cylinders with 20 random materials, the reference
// scene script's distributions (video_renderer.cpp:41-117), identical to scenes.scene_s1000.
void add_s1000(PathTracer& tracer, uint32_t seed = 20250124u, int n = 1000) {
    MsvcRand rng{seed};
    std::vector<Material> mats;
    mats.push_back(make_material(MaterialType::Diffuse, make_float3(0.95f, 0.95f, 0.95f)));
    for (int i = 1; i < 20; ++i) {
        const float3 kd = rng.random3();
        const int rnd = (int)(rng.random() * 2048.0f) % 5;
        if (rnd == 1) {
            const float sm = rng.random() * 4.0f + 1.0f;
            const float refl = rng.random() * 0.8f;
            mats.push_back(make_material(MaterialType::Metal, kd, 0.f, sm, refl));
        } else if (rnd == 2) {
            const float3 u = rng.random3();
            const float3 kd2 = make_float3(0.5f + 0.5f * u.x, 0.5f + 0.5f * u.y, 0.5f + 0.5f * u.z);
            mats.push_back(make_material(MaterialType::Mirror, kd2, 0.f, rng.random() * 4.0f + 0.5f));
        } else if (rnd == 3) {
            const float sm = rng.random() * 4.0f + 2.0f;
            const float ior = rng.random() * 2.0f + 1.2f;
            mats.push_back(make_material(MaterialType::Glass, make_float3(1.f, 1.f, 1.f), ior, sm));
        } else {
            mats.push_back(make_material(MaterialType::Diffuse, kd));
        }
    }
    Object* floor = make_object(PrimitiveType::Platform, mats[0], make_float3(0, -10000.f, 0), 10000.f, 0.f);
    add(tracer, floor);
    for (int k = 0; k < n; ++k) {
        const float z = -550.0f + 1.1f * (float)k;
        const int rnd = (int)(rng.random() * 2048.0f) % 2;
        const Material& mat = mats[rng.rand() % 20];
        const float r = rng.random() * 15.0f + 1.0f;
        if (rnd == 0) {
            const float x = rng.random() * 300.0f - 150.0f;
            add(tracer, make_object(PrimitiveType::Sphere, mat, make_float3(x, r, z), r, 0.f));
        } else {
            const float h = r / 2.0f + rng.random() * 20.0f;
            const float x = rng.random() * 300.0f - 150.0f;
            add(tracer, make_object(PrimitiveType::Cylinder, mat, make_float3(x, h / 2.0f, z), r, h));
        }
    }
}

struct FrameSink {
    std::atomic<int> frames{0};
    std::vector<uint8_t> last;
};

void on_frame(uint8_t* data, int width, int height, void* param) {
    FrameSink* s = static_cast<FrameSink*>(param);
    s->last.assign(data, data + (size_t)width * height * 4);
    s->frames++;
}

}  // namespace

int main(int argc, char** argv) {
    std::string scene = "s4", out, bgra_out, pfm, texture, dump_scene, pick;
    int W = 64, H = 36, spp = 2, depth = 8, dispatch = 0, devices = 1, n_objects = 1000, animate = 0;
    unsigned long long seed = 1234;
    // --adaptive REL: --spp is the most passes a pixel gets; tiles stop once their pixels'
    // relative standard error is at most REL (PathTracer::RenderAdaptive)
    float adaptive = -1.f;
    int min_spp = 0, batch = 0;
    // --filter [LEVELS] (with --adaptive): the variance-guided a-trous filter of the adaptive frame
    // (PathTracer::FilterRadiance, 5 levels by default); --pfm then gets the filtered image
    int filter_levels = -1;
    int orbit = 0;
    int filter_spatial = -1;   // --filter-spatial [LEVELS]: FilterRadianceSpatial on the last frame (-1: off)
    bool look_aside = false;   // --look-aside (with --filter-spatial): ReadGBuffer at a turned camera, then filter again
    int fill = 0;   // --fill T: frames after the first are topped up to T passes (0: --spp uniform passes)
    float animate_step = 0.75f;
    bool reproject = false;
    std::string display_reproject;   // "", "on" or "off"
    std::string present, exposure;   // --present clamp|reinhard|aces, --exposure auto|X
    bool present_linear = false;     // --linear: CPT_TRANSFER_LINEAR
    int aa = 0;                      // --aa 2|4: antialiased presentation
    std::string bloom;               // --bloom THRESHOLD[,LEVELS[,INTENSITY]]
    for (int i = 1; i < argc; i += 2) {
        std::string k = argv[i];
        if (k == "--filter") {
            const bool has_value = i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0;
            filter_levels = has_value ? std::stoi(argv[i + 1]) : 5;
            if (!has_value) --i;
            continue;
        }
        if (k == "--filter-spatial") {
            const bool has_value = i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0;
            filter_spatial = has_value ? std::stoi(argv[i + 1]) : 3;
            if (!has_value) --i;
            continue;
        }
        if (k == "--look-aside") {
            look_aside = true;
            --i;
            continue;
        }
        if (k == "--reproject") {
            reproject = true;
            --i;
            continue;
        }
        if (k == "--linear") {
            present_linear = true;
            --i;
            continue;
        }
        if (i + 1 >= argc) break;
        std::string v = argv[i + 1];
        if (k == "--scene") scene = v;
        else if (k == "--width") W = std::stoi(v);
        else if (k == "--height") H = std::stoi(v);
        else if (k == "--spp") spp = std::stoi(v);
        else if (k == "--depth") depth = std::stoi(v);
        else if (k == "--seed") seed = std::stoull(v);
        else if (k == "--out") out = v;
        else if (k == "--dispatch") dispatch = std::stoi(v);
        else if (k == "--bgra") bgra_out = v;
        else if (k == "--pfm") pfm = v;
        else if (k == "--texture") texture = v;
        else if (k == "--dump-scene") dump_scene = v;
        else if (k == "--devices") devices = std::stoi(v);
        else if (k == "--objects") n_objects = std::stoi(v);
        else if (k == "--animate") animate = std::stoi(v);
        else if (k == "--animate-step") animate_step = std::stof(v);
        else if (k == "--pick") pick = v;
        else if (k == "--orbit") orbit = std::stoi(v);
        else if (k == "--fill") fill = std::stoi(v);
        else if (k == "--display-reproject") display_reproject = v;
        else if (k == "--present") present = v;
        else if (k == "--exposure") exposure = v;
        else if (k == "--aa") aa = std::stoi(v);
        else if (k == "--bloom") bloom = v;
        else if (k == "--adaptive") adaptive = std::stof(v);
        else if (k == "--min-spp") min_spp = std::stoi(v);
        else if (k == "--batch") batch = std::stoi(v);
        else { fprintf(stderr, "unknown option %s\n", k.c_str()); return 2; }
    }

    PathTracer tracer;
    std::shared_ptr<MotionalCamera> cam(
        new MotionalCamera(W, H, make_float3(130.f, 103.f, 130.f), make_float3(0.f, 0.f, 0.f)));
    tracer.SetCamera(cam);
    tracer.SetSeed(seed);
    if (devices > 1 && !tracer.SetDevices(devices)) { fprintf(stderr, "%s\n", tracer.LastError().c_str()); return 1; }
    if (!tracer.SetMaxRecursionDepth((uint)depth)) { fprintf(stderr, "%s\n", tracer.LastError().c_str()); return 1; }

    // The same scenes as cpppathtracer_amd/scenes.py (S3, S4, S1000).
    if (scene == "s1000") {
        add_s1000(tracer, 20250124u, n_objects);
    } else if (scene == "s3") {
        add(tracer, make_sphere(make_material(MaterialType::Diffuse, make_float3(0.8f, 0.3f, 0.3f)), make_float3(-35.f, 15.f, 0.f), 15.f));
        add(tracer, make_sphere(make_material(MaterialType::Diffuse, make_float3(0.3f, 0.8f, 0.3f)), make_float3(0.f, 15.f, 0.f), 15.f));
        add(tracer, make_sphere(make_material(MaterialType::Diffuse, make_float3(0.3f, 0.3f, 0.8f)), make_float3(35.f, 15.f, 0.f), 15.f));
    } else {
        PocaTexture tex = 0;
        if (!texture.empty()) {
            tex = PocaTextureUtils::AddTexByFile(texture);
            if (!tex) return 1;
            printf("texture handle %llu\n", (unsigned long long)tex);
        }
        auto textured = [tex](Material m) {
            if (tex) { m.have_tex_ = true; m.tex_ = tex; }
            return m;
        };
        Object* floor = new Object();
        std::memset(floor, 0, sizeof(Object));
        floor->material_ = textured(make_material(MaterialType::Diffuse, make_float3(0.95f, 0.95f, 0.95f)));
        floor->type_ = PrimitiveType::Platform;
        floor->y_pos_ = 0.f;
        floor->center_ = make_float3(0, -10000.f, 0);
        floor->radius_ = 10000.f;
        add(tracer, floor);
        add(tracer, make_sphere(textured(make_material(MaterialType::Glass, make_float3(1.f), 1.5f, 4.f)), make_float3(-35.f, 15.f, 0.f), 15.f));
        add(tracer, make_sphere(textured(make_material(MaterialType::Metal, make_float3(0.8f, 0.6f, 0.2f), 0.f, 2.5f)), make_float3(0.f, 15.f, 0.f), 15.f));
        add(tracer, make_sphere(make_material(MaterialType::Mirror, make_float3(0.9f), 0.f, 3.f, 0.6f), make_float3(35.f, 15.f, 0.f), 15.f));
    }

    if (!dump_scene.empty()) {
        SceneBVH::BuildBVH();
        uint64_t build = 0, rev = 0;
        std::vector<cpt_object> built, current;
        std::vector<uint64_t> updates;
        SceneBVH::GetState(build, rev, &built, current, updates);
        std::ofstream f(dump_scene, std::ios::binary);
        f.write(reinterpret_cast<const char*>(built.data()), (std::streamsize)(built.size() * sizeof(cpt_object)));
        printf("dumped %zu objects\n", built.size());
        return f ? 0 : 1;
    }

    if (!pick.empty()) {
        int px = 0, py = 0;
        if (sscanf(pick.c_str(), "%d,%d", &px, &py) != 2) { fprintf(stderr, "--pick wants X,Y\n"); return 2; }
        float t = 0.f;
        const int object = tracer.Pick(px, py, &t);
        if (object < 0 && !tracer.LastError().empty()) { fprintf(stderr, "Pick: %s\n", tracer.LastError().c_str()); return 1; }
        printf("pick (%d, %d): object %d, t %.9g\n", px, py, object, (double)t);
        return 0;
    }

    if (fill != 0 && (fill < 1 || !reproject || (orbit <= 0 && animate <= 0))) {
        fprintf(stderr, "--fill wants T >= 1 and --reproject with --orbit N or --animate K\n");
        return 2;
    }
    if (filter_spatial >= 0 && (adaptive >= 0.f || animate > 0 || !display_reproject.empty() || (orbit > 0 && !reproject))) {
        fprintf(stderr, "--filter-spatial wants plain --spp or --orbit N --reproject [--fill T], without --adaptive\n");
        return 2;
    }
    if (look_aside && filter_spatial < 0) {
        fprintf(stderr, "--look-aside wants --filter-spatial\n");
        return 2;
    }
    int present_tone = -1;
    float present_exposure = 0.f;   // --exposure X (0: auto or none)
    if (!present.empty() || !exposure.empty() || present_linear) {
        present_tone = present == "clamp" ? CPT_TONE_CLAMP : present == "reinhard" ? CPT_TONE_REINHARD : present == "aces" ? CPT_TONE_ACES : -1;
        if (!exposure.empty() && exposure != "auto") present_exposure = std::stof(exposure);
        if (present_tone < 0 || !display_reproject.empty() || dispatch > 0 || adaptive >= 0.f || animate > 0 || (orbit > 0 && !reproject) ||
            bgra_out.empty() || (!exposure.empty() && exposure != "auto" && !(present_exposure > 0.f))) {
            fprintf(stderr, "--present wants clamp, reinhard or aces, --bgra, [--exposure auto|X > 0] [--linear], and plain --spp or "
                            "--orbit N --reproject [--fill T] [--filter-spatial]; not --display-reproject, --dispatch, --adaptive or --animate\n");
            return 2;
        }
    }
    if (aa != 0 && (present_tone < 0 || (aa != 2 && aa != 4))) {
        fprintf(stderr, "--aa wants 2 or 4, and --present\n");
        return 2;
    }
    float bloom_threshold = 0.f, bloom_intensity = 0.25f;
    int bloom_levels = 6;
    if (!bloom.empty()) {
        char end = 0;
        const int got = sscanf(bloom.c_str(), "%f,%d,%f%c", &bloom_threshold, &bloom_levels, &bloom_intensity, &end);
        if (present_tone < 0 || aa != 0 || got < 1 || got > 3 || !(bloom_threshold >= 0.f) || bloom_levels < 1 ||
            bloom_levels > CPT_BLOOM_MAX_LEVELS || !(bloom_intensity >= 0.f)) {
            fprintf(stderr, "--bloom wants THRESHOLD[,LEVELS[,INTENSITY]] (>= 0, 1..%d, >= 0) and --present, without --aa\n",
                    CPT_BLOOM_MAX_LEVELS);
            return 2;
        }
    }
    if (!display_reproject.empty()) {
        if (orbit <= 0 || (display_reproject != "on" && display_reproject != "off" && display_reproject != "edits")) {
            fprintf(stderr, "--display-reproject wants on, off or edits, and --orbit N\n");
            return 2;
        }
        FrameSink sink;
        if (!tracer.SetDisplayReprojection(display_reproject != "off", 32, 1e-2f, display_reproject == "edits")) {
            fprintf(stderr, "SetDisplayReprojection: %s\n", tracer.LastError().c_str());
            return 1;
        }
        tracer.InitPipeline();
        const float c = 0.99984770f, s = 0.01745241f;   // the orbit of --orbit below
        float dx = cam->origin_.x - cam->look_at_.x, dz = cam->origin_.z - cam->look_at_.z;
        int sent = 0;
        for (int f = 0; f < orbit + animate; ++f) {
            if (f > 0 && f < orbit) {
                const float nx = c * dx + s * dz, nz = c * dz - s * dx;
                dx = nx;
                dz = nz;
                cam->SetOrigin(cam->look_at_.x + dx, cam->origin_.y, cam->look_at_.z + dz);
                cam->Refresh();
            }
            if (f >= orbit)   // --animate: the camera stays, every tenth object moves (no Refresh)
                for (size_t i = 1; i < g_objects.size(); i += 10) {
                    g_objects[i]->center_.x += animate_step;
                    SceneBVH::UpdateObject(g_objects[i]);
                }
            for (int p = 0; p < spp; ++p) {
                tracer.DispatchRay(DispatchRayArgs{&sink, on_frame});
                ++sent;
                const auto t0 = std::chrono::steady_clock::now();
                while (sink.frames.load() < sent) {
                    std::this_thread::sleep_for(std::chrono::microseconds(200));
                    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) {
                        fprintf(stderr, "dispatch timeout (%s)\n", tracer.LastError().c_str());
                        return 1;
                    }
                }
            }
        }
        tracer.Stop();
        printf("orbit: %d cameras and %d edited frames of %d display passes, display reprojection %s\n", orbit, animate, spp,
               display_reproject.c_str());
        if (!bgra_out.empty()) {
            std::ofstream f(bgra_out, std::ios::binary);
            f.write(reinterpret_cast<const char*>(sink.last.data()), (std::streamsize)sink.last.size());
        }
        return 0;
    }

    if (dispatch > 0) {
        FrameSink sink;
        tracer.InitPipeline();
        for (int i = 0; i < dispatch; ++i) tracer.DispatchRay(DispatchRayArgs{&sink, on_frame});
        auto t0 = std::chrono::steady_clock::now();
        while (sink.frames.load() < dispatch) {
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) {
                fprintf(stderr, "dispatch timeout (%s)\n", tracer.LastError().c_str());
                return 1;
            }
        }
        tracer.Stop();
        printf("dispatched %d frames, cur_sample_idx %u\n", sink.frames.load(), cam->cur_sample_idx_);
        if (!bgra_out.empty()) {
            std::ofstream f(bgra_out, std::ios::binary);
            f.write(reinterpret_cast<const char*>(sink.last.data()), (std::streamsize)sink.last.size());
        }
        return 0;
    }

    if (adaptive >= 0.f) {
        // defaults: about 16 rounds (a batch that divides --spp), no tile stops before the second
        if (batch <= 0)
            for (batch = std::max(1, spp / 16); spp % batch; --batch) {}
        if (min_spp <= 0) min_spp = std::min(spp, 2 * batch);
        int rounds = 0;
        uint64_t passes = 0;
        if (!tracer.RenderAdaptive(min_spp, spp, batch, adaptive, &rounds, &passes)) {
            fprintf(stderr, "RenderAdaptive: %s\n", tracer.LastError().c_str());
            return 1;
        }
        printf("adaptive: rel_error %g, %d..%d spp in batches of %d: %d rounds, passes_done %llu (%.1f%% of %d spp)\n",
               (double)adaptive, min_spp, spp, batch, rounds, (unsigned long long)passes,
               100.0 * (double)passes / ((double)W * H * spp), spp);
        if (filter_levels >= 0) {
            if (!tracer.FilterRadiance(filter_levels)) { fprintf(stderr, "FilterRadiance: %s\n", tracer.LastError().c_str()); return 1; }
            printf("filtered: %d levels\n", filter_levels);
        }
    } else if (orbit > 0) {
        // one degree per frame about the vertical axis through the look-at point, in f32 as written
        const float c = 0.99984770f, s = 0.01745241f;
        float dx = cam->origin_.x - cam->look_at_.x, dz = cam->origin_.z - cam->look_at_.z;
        for (int f = 0; f < orbit; ++f) {
            const MotionalCamera from = *cam;   // the camera the accumulator was rendered with
            if (f > 0) {
                const float nx = c * dx + s * dz, nz = c * dz - s * dx;
                dx = nx;
                dz = nz;
                cam->SetOrigin(cam->look_at_.x + dx, cam->origin_.y, cam->look_at_.z + dz);
                if (reproject && !tracer.Reproject(from)) { fprintf(stderr, "Reproject: %s\n", tracer.LastError().c_str()); return 1; }
            }
            if (f > 0 && fill > 0) {
                if (!tracer.RenderToCount(fill)) { fprintf(stderr, "RenderToCount: %s\n", tracer.LastError().c_str()); return 1; }
            } else if (!tracer.Render(spp, f > 0)) { fprintf(stderr, "Render: %s\n", tracer.LastError().c_str()); return 1; }
        }
        printf("orbit: %d frames of %d spp%s", orbit, spp, reproject ? ", reprojected" : "");
        if (fill > 0) printf(", topped up to %d", fill);
        printf("\n");
    } else if (!tracer.Render(spp, false)) { fprintf(stderr, "Render: %s\n", tracer.LastError().c_str()); return 1; }
    if (animate > 0 && reproject && !tracer.CaptureHistory()) { fprintf(stderr, "CaptureHistory: %s\n", tracer.LastError().c_str()); return 1; }
    for (int f = 1; f <= animate; ++f) {
        const auto t0 = std::chrono::steady_clock::now();
        int moved = 0;
        for (size_t i = 1; i < g_objects.size(); i += 10) {
            g_objects[i]->center_.x += animate_step;
            SceneBVH::UpdateObject(g_objects[i]);
            ++moved;
        }
        // --reproject: the frames join one accumulator, its history following the moved objects
        if (reproject && !tracer.ReprojectTracked()) { fprintf(stderr, "ReprojectTracked: %s\n", tracer.LastError().c_str()); return 1; }
        if (fill > 0) {
            if (!tracer.RenderToCount(fill)) { fprintf(stderr, "RenderToCount: %s\n", tracer.LastError().c_str()); return 1; }
        } else if (!tracer.Render(spp, reproject)) { fprintf(stderr, "Render: %s\n", tracer.LastError().c_str()); return 1; }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("frame %d: %d objects moved, update + render %.3f ms\n", f, moved, ms);
    }
    std::vector<float> rgb;
    if (!tracer.ReadRadiance(rgb)) { fprintf(stderr, "ReadRadiance: %s\n", tracer.LastError().c_str()); return 1; }
    double mean = 0;
    for (float v : rgb) mean += v;
    printf("rendered %dx%d x %d spp (depth %d) on %d device context(s): mean radiance %.6f\n", W, H, spp, depth,
           tracer.DeviceCount(), mean / rgb.size());
    if (!out.empty()) {
        std::ofstream f(out, std::ios::binary);
        f.write(reinterpret_cast<const char*>(rgb.data()), (std::streamsize)(rgb.size() * sizeof(float)));
    }
    if (filter_spatial >= 0) {
        if (!tracer.FilterRadianceSpatial(filter_spatial)) { fprintf(stderr, "FilterRadianceSpatial: %s\n", tracer.LastError().c_str()); return 1; }
        printf("filtered without moments: %d levels\n", filter_spatial);
        if (look_aside) {
            const float c = 0.99984770f, s = 0.01745241f;
            const float dx = cam->origin_.x - cam->look_at_.x, dz = cam->origin_.z - cam->look_at_.z;
            cam->SetOrigin(cam->look_at_.x + (c * dx + s * dz), cam->origin_.y, cam->look_at_.z + (c * dz - s * dx));
            std::vector<int32_t> id;
            std::vector<float> t, normal3, albedo3;
            if (!tracer.ReadGBuffer(id, t, normal3, albedo3)) { fprintf(stderr, "ReadGBuffer: %s\n", tracer.LastError().c_str()); return 1; }
            if (!tracer.FilterRadianceSpatial(filter_spatial)) { fprintf(stderr, "FilterRadianceSpatial: %s\n", tracer.LastError().c_str()); return 1; }
            printf("looked aside (G-buffer at the turned camera) and filtered again\n");
        }
    }
    if (present_tone >= 0) {
        const bool from_filtered = filter_spatial >= 0;
        if (exposure == "auto" && !tracer.MeterExposure(from_filtered)) { fprintf(stderr, "MeterExposure: %s\n", tracer.LastError().c_str()); return 1; }
        if (present_exposure > 0.f && !tracer.SetExposure(present_exposure)) { fprintf(stderr, "SetExposure: %s\n", tracer.LastError().c_str()); return 1; }
        std::vector<uint8_t> frame;
        if (aa != 0) {
            if (!tracer.ResolveCoverage(aa)) { fprintf(stderr, "ResolveCoverage: %s\n", tracer.LastError().c_str()); return 1; }
            if (!tracer.PresentAntialiased(frame, present_tone, !present_linear, from_filtered)) { fprintf(stderr, "PresentAntialiased: %s\n", tracer.LastError().c_str()); return 1; }
        } else if (!bloom.empty()) {
            if (!tracer.BuildBloom(from_filtered, bloom_threshold, bloom_levels)) { fprintf(stderr, "BuildBloom: %s\n", tracer.LastError().c_str()); return 1; }
            if (!tracer.PresentBloom(frame, present_tone, !present_linear, from_filtered, 4.0f, bloom_intensity)) { fprintf(stderr, "PresentBloom: %s\n", tracer.LastError().c_str()); return 1; }
        } else if (!tracer.Present(frame, present_tone, !present_linear, from_filtered)) { fprintf(stderr, "Present: %s\n", tracer.LastError().c_str()); return 1; }
        std::ofstream f(bgra_out, std::ios::binary);
        f.write(reinterpret_cast<const char*>(frame.data()), (std::streamsize)frame.size());
        printf("presented: %s, %s, exposure %s\n", present.c_str(), present_linear ? "linear" : "sRGB", exposure.empty() ? "1" : exposure.c_str());
    }
    const bool filtered = filter_spatial >= 0 || (adaptive >= 0.f && filter_levels >= 0 && animate == 0);
    if (!pfm.empty() && !(filtered ? tracer.SaveFilteredPFM(pfm) : tracer.SaveRadiancePFM(pfm))) { fprintf(stderr, "%s\n", tracer.LastError().c_str()); return 1; }
    return 0;
}
