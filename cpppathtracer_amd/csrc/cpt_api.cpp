// cpt_api.cpp — the reference-shaped C++ construction API (include/cpppathtracer/*.h) on top
// of the C-ABI (include/cpt.h).  Host code only; every GPU operation goes through cpt_*.
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <sstream>

#include "../../include/cpppathtracer/path_tracer.h"

// ======================================================================================
// Object (object.cu:134-170)
// ======================================================================================
float3 Object::GetAABBMax() {
    float3 m = make_float3(0.f);
    const float tol = BOUNCE_RAY_TMIN * 5.f;
    switch (type_) {
        case PrimitiveType::Sphere: m = center_ + make_float3(ABS(radius_)); break;
        case PrimitiveType::Platform: m = make_float3(DEFAULT_RAY_TMAX * 5, y_pos_ + tol, DEFAULT_RAY_TMAX * 5); break;
        case PrimitiveType::Cylinder:
            m = make_float3(center_.x + ABS(radius_), center_.y + height_ / 2 + tol, center_.z + ABS(radius_));
            break;
        default: break;
    }
    return m;
}

float3 Object::GetAABBMin() {
    float3 m = make_float3(0.f);
    const float tol = BOUNCE_RAY_TMIN * 5.f;
    switch (type_) {
        case PrimitiveType::Sphere: m = center_ - make_float3(ABS(radius_)); break;
        case PrimitiveType::Platform: m = make_float3(-DEFAULT_RAY_TMAX * 5, y_pos_ - tol, -DEFAULT_RAY_TMAX * 5); break;
        case PrimitiveType::Cylinder:
            m = make_float3(center_.x - ABS(radius_), center_.y - height_ / 2 - tol, center_.z - ABS(radius_));
            break;
        default: break;
    }
    return m;
}

// ======================================================================================
// MotionalCamera (motional_camera.cu)
// ======================================================================================
static std::mutex camera_mutex;   // motional_camera.cu:12

MotionalCamera::MotionalCamera()
    : width_(1920), height_(1080), cur_sample_idx_(0), origin_(make_float3(0.f)), look_at_(make_float3(0.f, 0.f, 1.f)) {}
MotionalCamera::MotionalCamera(int width, int height)
    : width_(width), height_(height), cur_sample_idx_(0), origin_(make_float3(0.f)), look_at_(make_float3(0.f, 0.f, 1.f)) {}
MotionalCamera::MotionalCamera(int width, int height, float3 ori, float3 at)
    : width_(width), height_(height), cur_sample_idx_(0), origin_(ori), look_at_(at) {}
MotionalCamera::~MotionalCamera() {}

void MotionalCamera::Refresh() { cur_sample_idx_ = 0; }
void MotionalCamera::SetViewFov(float fov) { view_fov_ = fov; }
void MotionalCamera::Resize(int width, int height) { width_ = width; height_ = height; }
void MotionalCamera::SetOrigin(float3 ori) { origin_ = ori; }
void MotionalCamera::SetOrigin(float x, float y, float z) { origin_ = make_float3(x, y, z); }
void MotionalCamera::SetLookAt(float3 look_at) { look_at_ = look_at; }
void MotionalCamera::SetLookAt(float x, float y, float z) { look_at_ = make_float3(x, y, z); }

// Interactive camera controls (motional_camera.cu:76-168).  SURVEY.md §2 puts them outside
// the hot path; they are kept only so the public MotionalCamera API is complete.  This is an
// API-behaviour restatement: a move is origin/look_at += (k * move_speed) * axis along the
// eye's left / back / up axis (a negated axis for the opposite move, which rounds exactly as
// the reference's -=), and a turn re-normalises look_at onto the unit sphere around the eye,
// steps it along the eye's left or up axis and re-normalises, with the reference's float
// operations in the reference's order.
namespace {
float3 eye_left(const MotionalCamera& c) { return -normalize(cross(c.vup, normalize(c.origin_ - c.look_at_))); }
float3 eye_back(const MotionalCamera& c) { return -normalize(cross(eye_left(c), c.vup)); }

void translate(MotionalCamera& c, float3 axis, float k) {
    c.origin_ += k * c.move_speed_ * axis;
    c.look_at_ += k * c.move_speed_ * axis;
}

// `up`: step along the up axis (else the left axis) by d.
void turn(MotionalCamera& c, bool up, float d) {
    c.look_at_ = c.origin_ + normalize(c.look_at_ - c.origin_);
    const float3 w = normalize(c.look_at_ - c.origin_);
    const float3 left = normalize(cross(c.vup, w));
    const float3 axis = up ? normalize(cross(w, left)) : left;
    c.look_at_ += d * axis;
    c.look_at_ = c.origin_ + normalize(c.look_at_ - c.origin_);
}
}  // namespace

void MotionalCamera::MoveEyeLeft(float k) { translate(*this, eye_left(*this), k); }
void MotionalCamera::MoveEyeRight(float k) { translate(*this, -eye_left(*this), k); }
void MotionalCamera::MoveEyeForward(float k) { translate(*this, -eye_back(*this), k); }
void MotionalCamera::MoveEyeBackward(float k) { translate(*this, eye_back(*this), k); }
void MotionalCamera::MoveEyeUp(float k) { translate(*this, vup, k); }
void MotionalCamera::MoveEyeDown(float k) { translate(*this, -vup, k); }
void MotionalCamera::RotateAroundUp(float dy) { turn(*this, true, dy); }
void MotionalCamera::RotateAroundDown(float dy) { turn(*this, true, -dy); }
void MotionalCamera::RotateAroundLeft(float dx) { turn(*this, false, dx); }
void MotionalCamera::RotateAroundRight(float dx) { turn(*this, false, -dx); }
void MotionalCamera::ScaleFov(float d) { view_fov_ = (float)(view_fov_ + d * M_PI / 180.0f); }
void MotionalCamera::Lock() { camera_mutex.lock(); }
void MotionalCamera::Unlock() { camera_mutex.unlock(); }

MotionalCamera MotionalCamera::GetCopy() {
    std::lock_guard<std::mutex> lock(camera_mutex);
    cpt_camera_get_copy(reinterpret_cast<cpt_camera*>(this));   // basis + cur_sample_idx_++
    return *this;
}

// ======================================================================================
// SceneBVH statics (bvh.cu:16-29, 116-165)
// ======================================================================================
namespace {
std::mutex bvh_mutex;
std::vector<Object*> bvh_objs;
std::set<Object*> bvh_seen;
std::vector<cpt_object> bvh_built;      // BuildBVH's by-value copies (bvh.cu:43)
std::vector<cpt_object> bvh_current;    // ... with UpdateObject's re-copies
std::vector<uint64_t> bvh_updates;      // UpdateObject calls per object since the build
uint64_t bvh_build_id = 0, bvh_revision = 0;
SceneBVH* const bvh_handle = reinterpret_cast<SceneBVH*>(&bvh_built);   // opaque, non-null

// texture registry
std::mutex tex_mutex;
std::map<PocaTexture, PocaTextureData> tex_registry;
PocaTexture tex_next = 1;
}  // namespace

void SceneBVH::AddObject(Object* obj) {
    std::lock_guard<std::mutex> lk(bvh_mutex);
    if (obj == nullptr || bvh_seen.count(obj)) return;
    bvh_objs.push_back(obj);
    bvh_seen.insert(obj);
}

SceneBVHGPUHandle SceneBVH::BuildBVH() {
    std::lock_guard<std::mutex> lk(bvh_mutex);
    bvh_built.resize(bvh_objs.size());
    for (size_t i = 0; i < bvh_objs.size(); ++i) std::memcpy(&bvh_built[i], bvh_objs[i], sizeof(cpt_object));
    bvh_current = bvh_built;
    bvh_updates.assign(bvh_built.size(), 0);
    bvh_build_id++;
    bvh_revision++;
    return bvh_handle;
}

void SceneBVH::UpdateObject(Object* obj) {
    std::lock_guard<std::mutex> lk(bvh_mutex);
    for (size_t i = 0; i < bvh_objs.size() && i < bvh_current.size(); ++i)
        if (bvh_objs[i] == obj) {
            std::memcpy(&bvh_current[i], obj, sizeof(cpt_object));
            bvh_updates[i]++;
            bvh_revision++;
            return;
        }
}

void SceneBVH::ReleaseBVH() {
    std::lock_guard<std::mutex> lk(bvh_mutex);
    bvh_objs.clear();
    bvh_seen.clear();
    bvh_built.clear();
    bvh_current.clear();
    bvh_updates.clear();
    bvh_build_id++;
    bvh_revision++;
}

uint64_t SceneBVH::BuildId() {
    std::lock_guard<std::mutex> lk(bvh_mutex);
    return bvh_build_id;
}

uint64_t SceneBVH::Revision() {
    std::lock_guard<std::mutex> lk(bvh_mutex);
    return bvh_revision;
}

void SceneBVH::GetState(uint64_t& build_id, uint64_t& revision, std::vector<cpt_object>* built,
                        std::vector<cpt_object>& current, std::vector<uint64_t>& updates) {
    std::lock_guard<std::mutex> lk(bvh_mutex);
    build_id = bvh_build_id;
    revision = bvh_revision;
    if (built) *built = bvh_built;
    current = bvh_current;
    updates = bvh_updates;
}

int SceneBVH::IndexOf(const Object* obj) {
    std::lock_guard<std::mutex> lk(bvh_mutex);
    for (size_t i = 0; i < bvh_objs.size(); ++i)
        if (bvh_objs[i] == obj) return (int)i;
    return -1;
}

// ======================================================================================
// PocaTextureUtils (textures.cu:14-66)
// ======================================================================================
static bool load_cptex(const std::string& path, PocaTextureData& t) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    char magic[8];
    uint32_t hdr[4];
    if (!f.read(magic, 8) || std::memcmp(magic, "CPTTEX01", 8) != 0) return false;
    if (!f.read(reinterpret_cast<char*>(hdr), sizeof(hdr))) return false;
    t.width = (int)hdr[0];
    t.height = (int)hdr[1];
    t.valid_cols = (int)hdr[2];
    t.rgba.resize((size_t)t.valid_cols * t.height * 4);
    return (bool)f.read(reinterpret_cast<char*>(t.rgba.data()), (std::streamsize)t.rgba.size());
}

static bool load_ppm(const std::string& path, PocaTextureData& t) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::string magic;
    f >> magic;
    if (magic != "P6") return false;
    int w = 0, h = 0, maxv = 0;
    f >> w >> h >> maxv;
    f.get();
    if (w <= 0 || h <= 0 || maxv != 255) return false;
    std::vector<uint8_t> rgb((size_t)w * h * 3);
    if (!f.read(reinterpret_cast<char*>(rgb.data()), (std::streamsize)rgb.size())) return false;
    // textures.cu:32-33: cudaMemcpy2DToArray copies `width` BYTES per row = width/4 texels.
    t.width = w;
    t.height = h;
    t.valid_cols = w / 4;
    t.rgba.resize((size_t)t.valid_cols * h * 4);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < t.valid_cols; ++x) {
            const uint8_t* s = &rgb[((size_t)y * w + x) * 3];
            uint8_t* d = &t.rgba[((size_t)y * t.valid_cols + x) * 4];
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = 255;
        }
    return true;
}

static int address_mode_of(PocaAddressMode m) {
    switch (m) {
        case PocaAddressMode::Wrap: return CPT_ADDRESS_WRAP;
        case PocaAddressMode::Clamp: return CPT_ADDRESS_CLAMP;
        case PocaAddressMode::Border: return CPT_ADDRESS_BORDER;
        default: return CPT_ADDRESS_MIRROR;
    }
}

PocaTexture PocaTextureUtils::AddTexByFile(std::string file_path, PocaAddressMode addr_mode, PocaFilterMode filter_mode) {
    PocaTextureData t;
    t.addr = addr_mode;
    t.filter = filter_mode;
    if (!load_cptex(file_path, t) && !load_ppm(file_path, t)) {
        fprintf(stderr, "[cpt] AddTexByFile: cannot load %s (.cptex or binary PPM)\n", file_path.c_str());
        return 0;
    }
    std::lock_guard<std::mutex> lk(tex_mutex);
    PocaTexture h = tex_next++;
    tex_registry[h] = std::move(t);
    return h;
}

void PocaTextureUtils::DestroyTexture(PocaTexture tex) {
    std::lock_guard<std::mutex> lk(tex_mutex);
    tex_registry.erase(tex);
}

const PocaTextureData* PocaTextureUtils::Get(PocaTexture tex) {
    std::lock_guard<std::mutex> lk(tex_mutex);
    auto it = tex_registry.find(tex);
    return it == tex_registry.end() ? nullptr : &it->second;
}

// ======================================================================================
// PathTracer (path_tracer.cu:29-319)
// ======================================================================================
static std::string default_sky_path() {
    if (const char* e = getenv("CPT_SKY_PATH")) return e;
    {
        std::ifstream f("assets/sky.cptex");
        if (f) return "assets/sky.cptex";
    }
    Dl_info info;
    if (dladdr(reinterpret_cast<void*>(&default_sky_path), &info) && info.dli_fname) {
        std::string so = info.dli_fname;
        std::string dir = so.substr(0, so.find_last_of('/'));
        return dir + "/../assets/sky.cptex";
    }
    return "assets/sky.cptex";
}

PathTracer::PathTracer() {}

PathTracer::~PathTracer() {
    Stop();
    if (output_pinned_) (void)cpt_host_unregister(output_buffer_.data());
    for (Tile& t : tiles_)
        if (t.ctx) cpt_destroy(t.ctx);
    if (frame_) cpt_destroy(frame_);
}

bool PathTracer::Fail(const char* what, cpt_ctx* ctx) {
    if (!ctx) ctx = FrameCtx();
    err_ = std::string(what) + ": " + (ctx ? cpt_last_error(ctx) : cpt_last_error(nullptr));
    fprintf(stderr, "[cpt] %s\n", err_.c_str());   // the reference logs and continues
    return false;
}

void PathTracer::AddObject(Object* obj) { SceneBVH::AddObject(obj); }

void PathTracer::SetCamera(std::shared_ptr<MotionalCamera>& camera) { camera_ = camera; }
std::shared_ptr<MotionalCamera> PathTracer::GetCamera() { return camera_; }

bool PathTracer::SetMaxRecursionDepth(uint depth) {
    if (depth > MAX_RECURSION_DEPTH_SET) {
        err_ = "SetMaxRecursionDepth: depth must be <= 32";
        return false;
    }
    max_recursion_depth_ = depth;
    return true;
}

void PathTracer::SetSeed(uint64_t seed) {
    std::lock_guard<std::mutex> lk(mu_);
    seed_ = seed;
    for (Tile& t : tiles_) t.rng_ready = false;
}

bool PathTracer::SetDevice(int device) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!tiles_.empty()) {
        err_ = "SetDevice: the context already exists";
        return false;
    }
    device_ = device;
    device_list_.clear();
    return true;
}

bool PathTracer::SetDevices(int n) {
    if (n < 1) {
        err_ = "SetDevices: n must be >= 1";
        return false;
    }
    int visible = 0;
    if (cpt_get_device_count(&visible) != CPT_OK || visible < 1) {
        err_ = "SetDevices: no HIP device visible";
        return false;
    }
    std::vector<int> devs(n);
    for (int i = 0; i < n; ++i) devs[i] = i % visible;
    return SetDevices(devs);
}

bool PathTracer::SetDevices(const std::vector<int>& devices) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!tiles_.empty()) {
        err_ = "SetDevices: the contexts already exist";
        return false;
    }
    if (devices.empty()) {
        err_ = "SetDevices: empty device list";
        return false;
    }
    device_list_ = devices.size() > 1 ? devices : std::vector<int>{};
    device_ = devices[0];
    return true;
}

bool PathTracer::SetEnvTexture(PocaTexture tex) {
    std::lock_guard<std::mutex> lk(mu_);
    env_ = tex;
    for (Tile& t : tiles_) t.env_uploaded = false;
    return true;
}

// One context per device of the row tiling (a single one without SetDevices), plus, with
// several, the frame context on the first device that receives the gathered tiles.
bool PathTracer::EnsureContext() {
    if (!tiles_.empty()) return true;
    const std::vector<int> devs = device_list_.empty() ? std::vector<int>{device_} : device_list_;
    std::vector<Tile> tiles(devs.size());
    for (size_t i = 0; i < devs.size(); ++i) {
        tiles[i].device = devs[i];
        if (cpt_create(devs[i], &tiles[i].ctx) != CPT_OK) {
            tiles[i].ctx = nullptr;
            for (Tile& t : tiles)
                if (t.ctx) cpt_destroy(t.ctx);
            return Fail("cpt_create", nullptr);
        }
    }
    if (devs.size() > 1 && cpt_create(devs[0], &frame_) != CPT_OK) {
        frame_ = nullptr;
        for (Tile& t : tiles) cpt_destroy(t.ctx);
        return Fail("cpt_create", nullptr);
    }
    tiles_ = std::move(tiles);
    return true;
}

// Binds every material texture handle `objs` use that the context does not hold yet.
bool PathTracer::BindTextures(Tile& tile, const std::vector<cpt_object>& objs) {
    for (const cpt_object& o : objs) {
        if (!o.material.have_tex) continue;
        const uint64_t h = o.material.u.tex;
        if (std::find(tile.bound_textures.begin(), tile.bound_textures.end(), h) != tile.bound_textures.end()) continue;
        const PocaTextureData* t = PocaTextureUtils::Get(h);
        if (!t) { err_ = "textured material uses an unknown PocaTexture handle"; return false; }
        if (cpt_bind_texture(tile.ctx, h, t->rgba.data(), t->width, t->height, t->valid_cols, address_mode_of(t->addr),
                             t->filter == PocaFilterMode::Point ? CPT_FILTER_POINT : CPT_FILTER_LINEAR) != CPT_OK)
            return Fail("cpt_bind_texture", tile.ctx);
        tile.bound_textures.push_back(h);
    }
    return true;
}

// Brings one context to a snapshot of SceneBVH's state: a new build is uploaded as BuildBVH
// copied it (the reference's topology), then the objects UpdateObject re-copied since are refit
// in one batch (bvh.cu:144-157).
bool PathTracer::SyncTile(Tile& tile, const SceneSnap& snap) {
    if (!tile.scene_synced || snap.rev != tile.scene_rev) {
        if (!tile.scene_synced || snap.build != tile.scene_build) {
            tile.bound_textures.clear();
            if (!BindTextures(tile, snap.built)) return false;
            if (cpt_set_scene(tile.ctx, snap.built.empty() ? nullptr : snap.built.data(), (int)snap.built.size()) != CPT_OK)
                return Fail("cpt_set_scene", tile.ctx);
            tile.scene_build = snap.build;
            tile.updates_seen.assign(snap.built.size(), 0);
        }
        std::vector<int> idx;
        std::vector<cpt_object> objs;
        for (size_t i = 0; i < snap.updates.size() && i < tile.updates_seen.size(); ++i)
            if (snap.updates[i] != tile.updates_seen[i]) {
                idx.push_back((int)i);
                objs.push_back(snap.current[i]);
            }
        if (!idx.empty()) {
            if (!BindTextures(tile, objs)) return false;
            if (cpt_update_objects(tile.ctx, (int)idx.size(), idx.data(), objs.data()) != CPT_OK)
                return Fail("cpt_update_objects", tile.ctx);
        }
        tile.updates_seen = snap.updates;
        tile.scene_rev = snap.rev;
        tile.scene_synced = true;
    }
    if (!tile.env_uploaded) {
        if (env_ == 0) env_ = PocaTextureUtils::AddTexByFile(default_sky_path());   // path_tracer.cu:47
        const PocaTextureData* t = PocaTextureUtils::Get(env_);
        int rc = t ? cpt_set_env_texture(tile.ctx, t->rgba.data(), t->width, t->height, t->valid_cols)
                   : cpt_set_env_texture(tile.ctx, nullptr, 1, 1, 0);
        if (rc != CPT_OK) return Fail("cpt_set_env_texture", tile.ctx);
        tile.env_uploaded = true;
    }
    return true;
}

// One snapshot for the whole pass: an UpdateObject from another thread lands either before
// every tile or after all of them, never between two tiles of one frame.
bool PathTracer::SyncScene() {
    if (!EnsureContext()) return false;
    SceneSnap snap;
    bool need = false;
    const uint64_t rev = SceneBVH::Revision();
    for (const Tile& t : tiles_) need = need || !t.scene_synced || t.scene_rev != rev;
    if (need) {
        SceneBVH::GetState(snap.build, snap.rev, &snap.built, snap.current, snap.updates);
    } else {
        snap.build = tiles_[0].scene_build;
        snap.rev = tiles_[0].scene_rev;
    }
    for (Tile& t : tiles_)
        if (!SyncTile(t, snap)) return false;
    return true;
}

// Image rows of tile r of n: interleaved 8-row blocks (cpppathtracer_amd/tiling.py).
static std::vector<int32_t> tile_rows(int height, int n, int r) {
    std::vector<int32_t> rows;
    for (int y = 0; y < height; ++y)
        if ((y / 8) % n == r) rows.push_back(y);
    return rows;
}

// InitBuffers (path_tracer.cu:44-115): per-pixel buffers and RNG when the size changes.
bool PathTracer::EnsureFrame(const MotionalCamera& cam) {
    const int n = (int)tiles_.size();
    if (cam.width_ != width_ || cam.height_ != height_) {
        for (int r = 0; r < n; ++r) {
            const std::vector<int32_t> rows = tile_rows(cam.height_, n, r);
            const int rc = n == 1 ? cpt_set_frame(tiles_[r].ctx, cam.width_, cam.height_, nullptr, 0)
                                  : cpt_set_frame(tiles_[r].ctx, cam.width_, cam.height_, rows.data(), (int)rows.size());
            if (rc != CPT_OK) return Fail("cpt_set_frame", tiles_[r].ctx);
            accum_cam_set_ = gbuffer_known_ = false;   // a fresh frame: no radiance, no G-buffer
            tiles_[r].rng_ready = false;
        }
        if (frame_ && cpt_set_frame(frame_, cam.width_, cam.height_, nullptr, 0) != CPT_OK) return Fail("cpt_set_frame", frame_);
        width_ = cam.width_;
        height_ = cam.height_;
        if (output_pinned_) (void)cpt_host_unregister(output_buffer_.data());
        output_buffer_.assign((size_t)width_ * height_ * 4, 0);
        // pinned, so each pass's frame reaches it without a staging copy (cpt_denoise_mix); a
        // buffer that cannot be pinned still works through the copy
        output_pinned_ = !output_buffer_.empty() &&
                         cpt_host_register(output_buffer_.data(), output_buffer_.size()) == CPT_OK;
    }
    for (Tile& t : tiles_)
        if (!t.rng_ready) {
            if (cpt_init_rng(t.ctx, seed_) != CPT_OK) return Fail("cpt_init_rng", t.ctx);
            t.rng_ready = true;
        }
    return true;
}

// One render of `spp` passes: every tile's launch is queued first (each context's work runs on
// its own device and stream), then the tiles are gathered into the frame context.
static MotionalCamera query_camera(const MotionalCamera& cam);

// `cam` as FilterRadianceSpatial's records keep it: the basis computed, the sample index (which no
// first hit depends on) cleared, so that two copies of one camera compare equal byte for byte.
static MotionalCamera record_camera(const MotionalCamera& cam) {
    MotionalCamera c = query_camera(cam);
    c.cur_sample_idx_ = 0;
    return c;
}

// The accumulator now belongs to `cam` (FilterRadianceSpatial).
void PathTracer::NoteAccumCamera(const MotionalCamera& cam) {
    accum_cam_ = record_camera(cam);
    accum_cam_set_ = true;
}

// The first tile's frame G-buffer now holds `cam`'s first hits in the scene as that tile has it.
void PathTracer::NoteGBuffer(const MotionalCamera& cam) {
    gbuffer_cam_ = record_camera(cam);
    gbuffer_rev_ = tiles_[0].scene_rev;
    gbuffer_known_ = true;
}

bool PathTracer::RenderPass(MotionalCamera& cam, int spp, bool accumulate) {
    if (!SyncScene() || !EnsureFrame(cam)) return false;
    NoteAccumCamera(cam);
    // many passes per pixel: heaviest tiles first (same image, shorter tail)
    // few passes (the DispatchRay loop): heaviest tiles first by the previous pass's work, no pilot
    const uint32_t flags = CPT_RENDER_AUX | (accumulate ? CPT_RENDER_ACCUMULATE : 0u) |
                           (ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u) |
                           (spp >= 64 ? CPT_SCHEDULE_COST : CPT_SCHEDULE_PREVIOUS);
    if (!frame_) {
        if (cpt_render(tiles_[0].ctx, reinterpret_cast<const cpt_camera*>(&cam), spp, (int)max_recursion_depth_,
                       flags | CPT_RENDER_SYNC) != CPT_OK)
            return Fail("cpt_render", tiles_[0].ctx);
        return true;
    }
    for (Tile& t : tiles_)
        if (cpt_render(t.ctx, reinterpret_cast<const cpt_camera*>(&cam), spp, (int)max_recursion_depth_, flags) != CPT_OK)
            return Fail("cpt_render", t.ctx);
    // every gather queues behind its tile's render (events, no host wait); one wait at the end
    for (Tile& t : tiles_)
        if (cpt_gather_rows(frame_, t.ctx) != CPT_OK) return Fail("cpt_gather_rows", frame_);
    if (cpt_synchronize(frame_) != CPT_OK) return Fail("cpt_synchronize", frame_);
    for (Tile& t : tiles_)   // the tiles' device errors (their work is done by now)
        if (cpt_synchronize(t.ctx) != CPT_OK) return Fail("cpt_synchronize", t.ctx);
    return true;
}

void PathTracer::InitPipeline() {
    SceneBVH::BuildBVH();   // bvh.cu:116-120
    if (running_.exchange(true)) return;
    worker_ = std::thread(&PathTracer::PipelineLoop, this);
}

void PathTracer::DispatchRay(DispatchRayArgs args) {
    {
        std::lock_guard<std::mutex> lk(mu_);
        tasks_queue_.push_back(args);
    }
    cv_.notify_one();
}

// PipelineLoop (path_tracer.cu:256-306): one sample per pixel per task, then denoise + mix and
// the callback with the BGRA8 frame, on this thread.
void PathTracer::PipelineLoop() {
    if (camera_) {
        MotionalCamera first = camera_->GetCopy();   // the reference's InitBuffers(GetCopy()) (:258)
        std::lock_guard<std::mutex> lk(mu_);
        if (SyncScene()) EnsureFrame(first);
    }
    while (running_.load()) {
        DispatchRayArgs task;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return !tasks_queue_.empty() || !running_.load(); });
            if (!running_.load()) break;
            task = tasks_queue_.front();
            tasks_queue_.pop_front();
        }
        if (!camera_) continue;
        MotionalCamera cma = camera_->GetCopy();
        bool ok;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (display_reproject_) {
                ok = DisplayPassWithHistory(cma);
            } else {
                ok = RenderPass(cma, 1, false);
                if (ok && cpt_denoise_mix(FrameCtx(), cma.cur_sample_idx_, output_buffer_.data()) != CPT_OK)
                    ok = Fail("cpt_denoise_mix");
            }
        }
        if (ok && task.Callback) task.Callback(output_buffer_.data(), width_, height_, task.cbParam);
    }
}

bool PathTracer::SetDisplayReprojection(bool on, int max_history, float plane_tol, bool through_edits) {
    std::lock_guard<std::mutex> lk(mu_);
    // what cpt_reproject_display would refuse at every Refresh is refused here, once
    if (max_history < 1 || !(plane_tol >= 0.f) || !(plane_tol - plane_tol == 0.f)) {
        err_ = "SetDisplayReprojection: max_history " + std::to_string(max_history) + " (>= 1), plane_tol " +
               std::to_string(plane_tol) + " (finite, >= 0)";
        return false;
    }
    display_reproject_ = on;
    display_through_edits_ = on && through_edits;
    loop_history_ = false;   // whatever history the context holds is not this loop's
    display_max_history_ = max_history;
    display_plane_tol_ = plane_tol;
    prev_pass_ = false;   // the first pass after a switch restarts
    return true;
}

// One pass of the loop with SetDisplayReprojection on (mu_ held): after a Refresh the display
// state moves to the new camera, or restarts where it cannot; then the pass and the per-pixel Mix.
// A pass that neither follows a Refresh nor a pass of this kind joins the mean the loop has so far
// through cpt_denoise_mix at the camera's index, which the per-pixel counts then continue from: the
// loop's first pass is such a one, its index being 2 after InitBuffers' copy (path_tracer.cu:258),
// so a still camera's frames are the reference loop's.
bool PathTracer::DisplayPassWithHistory(MotionalCamera& cma) {
    const bool had_prev = prev_pass_, refreshed = cma.cur_sample_idx_ == 1;
    prev_pass_ = false;
    const uint32_t walk = ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u;
    // (a frame under 16 pixels either way has no launch region: no display pass ever ran there)
    auto prev_fits = [&] {
        return had_prev && prev_cam_.width_ == width_ && prev_cam_.height_ == height_ && width_ >= 16 && height_ >= 16 && !frame_;
    };
    // through_edits.  The context's captured history serves this loop only while it is the previous
    // pass's: captured or renewed by this loop (loop_history_; Reproject, CaptureHistory,
    // ReprojectTracked and SetDisplayReprojection clear it, the untracked C calls drop the capture
    // itself), at the scene revision of the previous pass, and at a camera that equals prev_cam_ in
    // every field but the sample index.  Anything else is not trusted: the history is captured anew
    // at the previous pass's camera where the context still holds that pass's scene, and the display
    // restarts where it does not.
    if (!had_prev) loop_history_ = false;
    auto history_is_prev = [&](cpt_ctx* ctx, bool& is_prev) {
        int valid = 0;
        cpt_camera cam;
        is_prev = false;
        if (cpt_history_info(ctx, &valid, &cam) != CPT_OK) return false;
        if (valid && loop_history_ && loop_history_rev_ == prev_scene_rev_) {
            cpt_camera prev = *reinterpret_cast<const cpt_camera*>(&prev_cam_);
            prev.cur_sample_idx = cam.cur_sample_idx;
            is_prev = std::memcmp(&prev, &cam, sizeof(cam)) == 0;
        }
        return true;
    };
    // A move or an edit is about to reach the context: capture before SyncScene lets it.  (Revision()
    // is read before SyncScene reads it again: an UpdateObject from another thread that lands
    // between the two is not seen here, no capture is made for it, and the pass below then finds an
    // edited scene without a history of the previous pass and restarts the display.  Safe, but a
    // restart that through_edits would otherwise have avoided.)
    if (display_through_edits_ && prev_fits() && !tiles_.empty() && tiles_[0].scene_synced &&
        (refreshed || SceneBVH::Revision() != tiles_[0].scene_rev || tiles_[0].scene_rev != prev_scene_rev_)) {
        cpt_ctx* ctx = tiles_[0].ctx;
        bool is_prev = false;
        if (!history_is_prev(ctx, is_prev)) return Fail("cpt_history_info", ctx);
        if (!is_prev) {
            loop_history_ = false;
            // (edits another call already brought to the context cannot be captured behind)
            if (tiles_[0].scene_build == prev_scene_build_ && tiles_[0].scene_rev == prev_scene_rev_) {
                gbuffer_known_ = false;   // the capture traces the frame's G-buffer
                if (cpt_history_capture(ctx, reinterpret_cast<const cpt_camera*>(&prev_cam_), walk) != CPT_OK)
                    return Fail("cpt_history_capture", ctx);
                loop_history_ = true;
                loop_history_rev_ = prev_scene_rev_;
            }
        }
    }
    if (!SyncScene() || !EnsureFrame(cma)) return false;
    const Tile& t0 = tiles_[0];
    const bool same_build = t0.scene_build == prev_scene_build_, same_rev = t0.scene_rev == prev_scene_rev_;
    const bool edited = display_through_edits_ && had_prev && same_build && !same_rev;
    if (refreshed || edited) {
        bool carry = prev_fits() && same_build && (same_rev || display_through_edits_);
        if (carry && display_through_edits_) {
            // dropped by a new frame or scene, never captured, or not the previous pass's: restart
            if (!history_is_prev(t0.ctx, carry)) return Fail("cpt_history_info", t0.ctx);
        }
        if (carry) gbuffer_known_ = false;   // both reprojection calls trace the frame's G-buffer
        if (carry && display_through_edits_) {
            if (cpt_reproject_display_tracked(t0.ctx, reinterpret_cast<const cpt_camera*>(&cma), display_max_history_,
                                              display_plane_tol_, walk) != CPT_OK)
                return Fail("cpt_reproject_display_tracked", t0.ctx);
            loop_history_rev_ = t0.scene_rev;   // the call renewed the history: cma, the current objects
        } else if (carry) {
            if (cpt_reproject_display(t0.ctx, reinterpret_cast<const cpt_camera*>(&prev_cam_), reinterpret_cast<const cpt_camera*>(&cma),
                                      display_max_history_, display_plane_tol_, walk) != CPT_OK)
                return Fail("cpt_reproject_display", t0.ctx);
        } else {
            loop_history_ = false;
            if (cpt_reset_display(FrameCtx()) != CPT_OK) return Fail("cpt_reset_display");
        }
    }
    if (!RenderPass(cma, 1, false)) return false;
    if (!refreshed && !had_prev) {
        if (cpt_denoise_mix(FrameCtx(), cma.cur_sample_idx_, output_buffer_.data()) != CPT_OK) return Fail("cpt_denoise_mix");
    } else if (cpt_denoise_mix_history(FrameCtx(), output_buffer_.data()) != CPT_OK) {
        return Fail("cpt_denoise_mix_history");
    }
    prev_cam_ = cma;
    prev_scene_build_ = tiles_[0].scene_build;
    prev_scene_rev_ = tiles_[0].scene_rev;
    prev_pass_ = true;
    return true;
}

void PathTracer::Stop() {
    if (!running_.exchange(false)) return;
    cv_.notify_all();
    if (worker_.joinable()) worker_.join();
}

bool PathTracer::Render(int spp, bool accumulate) {
    if (!camera_) {
        err_ = "Render: SetCamera first";
        return false;
    }
    if (SceneBVH::BuildId() == 0) SceneBVH::BuildBVH();
    MotionalCamera cma = camera_->GetCopy();
    std::lock_guard<std::mutex> lk(mu_);
    return RenderPass(cma, spp, accumulate);
}

// Top-up render (cpt_render_to_count): as RenderPass, every row tile on its own
// accumulator, then the gather.
bool PathTracer::RenderToCount(int target) {
    if (!camera_) {
        err_ = "RenderToCount: SetCamera first";
        return false;
    }
    if (SceneBVH::BuildId() == 0) SceneBVH::BuildBVH();
    MotionalCamera cam = camera_->GetCopy();
    std::lock_guard<std::mutex> lk(mu_);
    if (!SyncScene() || !EnsureFrame(cam)) return false;
    NoteAccumCamera(cam);
    const uint32_t flags = CPT_RENDER_AUX | (ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u);
    const cpt_camera* c = reinterpret_cast<const cpt_camera*>(&cam);
    if (!frame_) {
        if (cpt_render_to_count(tiles_[0].ctx, c, target, (int)max_recursion_depth_, flags | CPT_RENDER_SYNC) != CPT_OK)
            return Fail("cpt_render_to_count", tiles_[0].ctx);
        return true;
    }
    for (Tile& t : tiles_)
        if (cpt_render_to_count(t.ctx, c, target, (int)max_recursion_depth_, flags) != CPT_OK)
            return Fail("cpt_render_to_count", t.ctx);
    for (Tile& t : tiles_)
        if (cpt_gather_rows(frame_, t.ctx) != CPT_OK) return Fail("cpt_gather_rows", frame_);
    if (cpt_synchronize(frame_) != CPT_OK) return Fail("cpt_synchronize", frame_);
    for (Tile& t : tiles_)   // the tiles' device errors (their work is done by now)
        if (cpt_synchronize(t.ctx) != CPT_OK) return Fail("cpt_synchronize", t.ctx);
    return true;
}

// The adaptive render over row tiles: every tile's first round is queued, then this thread goes
// round the unfinished tiles, each step reading one tile's round and queueing its next, so every
// device has a round queued while the host waits on another.  The tiles are whole 8-row blocks, so
// each tile's 8x8 tiles are the monolithic frame's and stop at the monolithic frame's rounds.
bool PathTracer::RenderAdaptiveTiles(MotionalCamera& cam, int min_spp, int max_spp, int batch, float rel_error,
                                     uint32_t flags, int* rounds, uint64_t* passes_done) {
    const size_t n = tiles_.size();
    std::vector<char> pending(n, 0);
    // a failure leaves no tile pending: the others' rounds are run to their end (a failed step
    // ends its own)
    auto fail_all = [&](const char* what, cpt_ctx* ctx) {
        Fail(what, ctx);
        for (size_t i = 0; i < n; ++i)
            for (int active = 1; pending[i] && active > 0;)
                if (cpt_adaptive_step(tiles_[i].ctx, &active) != CPT_OK) break;
        return false;
    };
    for (size_t i = 0; i < n; ++i) {
        if (cpt_adaptive_begin(tiles_[i].ctx, reinterpret_cast<const cpt_camera*>(&cam), min_spp, max_spp, batch, rel_error,
                               (int)max_recursion_depth_, flags) != CPT_OK)
            return fail_all("cpt_adaptive_begin", tiles_[i].ctx);
        pending[i] = 1;
    }
    for (size_t left = n; left > 0;)
        for (size_t i = 0; i < n; ++i) {
            if (!pending[i]) continue;
            int active = 0;
            if (cpt_adaptive_step(tiles_[i].ctx, &active) != CPT_OK) {
                pending[i] = 0;
                return fail_all("cpt_adaptive_step", tiles_[i].ctx);
            }
            if (active == 0) {
                pending[i] = 0;
                --left;
            }
        }
    for (Tile& t : tiles_)
        if (cpt_gather_rows(frame_, t.ctx) != CPT_OK) return Fail("cpt_gather_rows", frame_);
    if (cpt_synchronize(frame_) != CPT_OK) return Fail("cpt_synchronize", frame_);
    int most = 0;
    uint64_t sum = 0;
    for (Tile& t : tiles_) {
        if (cpt_synchronize(t.ctx) != CPT_OK) return Fail("cpt_synchronize", t.ctx);
        int r = 0;
        uint64_t p = 0;
        if (cpt_adaptive_info(t.ctx, &r, nullptr, 0, &p) != CPT_OK) return Fail("cpt_adaptive_info", t.ctx);
        most = std::max(most, r);
        sum += p;
    }
    if (rounds) *rounds = most;
    if (passes_done) *passes_done = sum;
    return true;
}

bool PathTracer::RenderAdaptive(int min_spp, int max_spp, int batch, float rel_error, int* rounds,
                                uint64_t* passes_done) {
    if (!camera_) {
        err_ = "RenderAdaptive: SetCamera first";
        return false;
    }
    if (SceneBVH::BuildId() == 0) SceneBVH::BuildBVH();
    MotionalCamera cma = camera_->GetCopy();
    std::lock_guard<std::mutex> lk(mu_);
    if (!SyncScene() || !EnsureFrame(cma)) return false;
    NoteAccumCamera(cma);   // for the row tiles too (RenderAdaptiveTiles)
    const uint32_t flags = CPT_RENDER_AUX | (ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u) |
                           (max_spp >= 64 ? CPT_SCHEDULE_COST : 0u);
    if (frame_) return RenderAdaptiveTiles(cma, min_spp, max_spp, batch, rel_error, flags, rounds, passes_done);
    cpt_ctx* ctx = tiles_[0].ctx;
    if (cpt_render_adaptive(ctx, reinterpret_cast<const cpt_camera*>(&cma), min_spp, max_spp, batch, rel_error,
                            (int)max_recursion_depth_, flags) != CPT_OK)
        return Fail("cpt_render_adaptive", ctx);
    if (cpt_adaptive_info(ctx, rounds, nullptr, 0, passes_done) != CPT_OK) return Fail("cpt_adaptive_info", ctx);
    return true;
}

bool PathTracer::ReadNoise(float* rel) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!FrameCtx() || width_ == 0) {
        err_ = "ReadNoise: RenderAdaptive first";
        return false;
    }
    if (cpt_read_noise(FrameCtx(), rel, (size_t)width_ * height_) != CPT_OK) return Fail("cpt_read_noise");
    return true;
}

bool PathTracer::FilterRadiance(int levels, float sigma_l, int sharpness) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!FrameCtx() || width_ == 0) {
        err_ = "FilterRadiance: RenderAdaptive first";
        return false;
    }
    if (cpt_filter_frame(FrameCtx(), levels, sigma_l, sharpness) != CPT_OK) return Fail("cpt_filter_frame");
    return true;
}

bool PathTracer::FilterRadianceSpatial(int levels, float sigma_l, int sharpness) {
    std::lock_guard<std::mutex> lk(mu_);
    if (tiles_.empty() || width_ == 0 || !accum_cam_set_) {
        err_ = "FilterRadianceSpatial: Render first";
        return false;
    }
    if (frame_) {
        err_ = "FilterRadianceSpatial: not available with SetDevices(n > 1), the row tiles own their G-buffers";
        return false;
    }
    cpt_ctx* ctx = tiles_[0].ctx;
    // the G-buffer the context holds is reused only if it is the accumulator's camera's, in the
    // scene the context has now
    if (!gbuffer_known_ || gbuffer_rev_ != tiles_[0].scene_rev || std::memcmp(&gbuffer_cam_, &accum_cam_, sizeof(accum_cam_)) != 0) {
        gbuffer_known_ = false;
        if (cpt_gbuffer(ctx, reinterpret_cast<const cpt_camera*>(&accum_cam_), ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u) != CPT_OK)
            return Fail("cpt_gbuffer", ctx);
        NoteGBuffer(accum_cam_);
    }
    if (cpt_filter_frame_spatial(ctx, levels, sigma_l, sharpness) != CPT_OK) return Fail("cpt_filter_frame_spatial", ctx);
    return true;
}

bool PathTracer::ReadFiltered(std::vector<float>& rgb) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!FrameCtx() || width_ == 0) {
        err_ = "ReadFiltered: FilterRadiance first";
        return false;
    }
    rgb.resize((size_t)width_ * height_ * 3);
    if (cpt_read_filtered(FrameCtx(), rgb.data(), nullptr, (size_t)width_ * height_) != CPT_OK)
        return Fail("cpt_read_filtered");
    return true;
}

bool PathTracer::ReadRadiance(std::vector<float>& rgb) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!FrameCtx() || width_ == 0) {
        err_ = "ReadRadiance: nothing rendered";
        return false;
    }
    std::vector<float> acc((size_t)width_ * height_ * 4);
    if (cpt_read_accum(FrameCtx(), acc.data()) != CPT_OK) return Fail("cpt_read_accum");
    rgb.resize((size_t)width_ * height_ * 3);
    for (size_t i = 0; i < (size_t)width_ * height_; ++i) {
        float n = acc[4 * i + 3] > 0.f ? acc[4 * i + 3] : 1.f;
        rgb[3 * i] = acc[4 * i] / n;
        rgb[3 * i + 1] = acc[4 * i + 1] / n;
        rgb[3 * i + 2] = acc[4 * i + 2] / n;
    }
    return true;
}

bool PathTracer::ReadFrameBGRA(std::vector<uint8_t>& bgra) {
    std::lock_guard<std::mutex> lk(mu_);
    bgra = output_buffer_;
    return !bgra.empty();
}

static bool write_pfm(const std::string& path, const std::vector<float>& rgb, int width, int height) {
    std::ofstream f(path, std::ios::binary);
    if (!f) return false;
    f << "PF\n" << width << " " << height << "\n-1.0\n";
    for (int y = height - 1; y >= 0; --y)   // PFM rows are bottom-to-top
        f.write(reinterpret_cast<const char*>(&rgb[(size_t)y * width * 3]), (std::streamsize)width * 3 * sizeof(float));
    return (bool)f;
}

bool PathTracer::SaveRadiancePFM(const std::string& path) {
    std::vector<float> rgb;
    if (!ReadRadiance(rgb)) return false;
    if (write_pfm(path, rgb, width_, height_)) return true;
    err_ = "SaveRadiancePFM: cannot write " + path;
    return false;
}

bool PathTracer::SaveFilteredPFM(const std::string& path) {
    std::vector<float> rgb;
    if (!ReadFiltered(rgb)) return false;
    if (write_pfm(path, rgb, width_, height_)) return true;
    err_ = "SaveFilteredPFM: cannot write " + path;
    return false;
}

// The current camera with its basis computed, as GetCopy() gives it, but from a copy: the
// camera's own sample index (the display path's Mix weight) does not move for a query.
static MotionalCamera query_camera(const MotionalCamera& cam) {
    MotionalCamera c = cam;
    cpt_camera_get_copy(reinterpret_cast<cpt_camera*>(&c));
    return c;
}

int PathTracer::Pick(int x, int y, float* t) {
    if (!camera_) {
        err_ = "Pick: SetCamera first";
        return -1;
    }
    if (SceneBVH::BuildId() == 0) SceneBVH::BuildBVH();
    const MotionalCamera cma = query_camera(*camera_);
    std::lock_guard<std::mutex> lk(mu_);
    if (!SyncScene() || !EnsureFrame(cma)) return -1;
    int32_t object = -1;
    if (cpt_pick(tiles_[0].ctx, reinterpret_cast<const cpt_camera*>(&cma), x, y, ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u,
                 &object, t) != CPT_OK) {
        Fail("cpt_pick", tiles_[0].ctx);
        return -1;
    }
    return object;
}

// Every tile's G-buffer is queued first, then each is read into its rows of the frame.
bool PathTracer::ReadGBuffer(std::vector<int32_t>& id, std::vector<float>& t, std::vector<float>& normal3,
                             std::vector<float>& albedo3) {
    if (!camera_) {
        err_ = "ReadGBuffer: SetCamera first";
        return false;
    }
    if (SceneBVH::BuildId() == 0) SceneBVH::BuildBVH();
    const MotionalCamera cma = query_camera(*camera_);
    std::lock_guard<std::mutex> lk(mu_);
    if (!SyncScene() || !EnsureFrame(cma)) return false;
    const uint32_t flags = ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u;
    gbuffer_known_ = false;
    for (Tile& tile : tiles_)
        if (cpt_gbuffer(tile.ctx, reinterpret_cast<const cpt_camera*>(&cma), flags) != CPT_OK)
            return Fail("cpt_gbuffer", tile.ctx);
    NoteGBuffer(cma);
    const size_t w = (size_t)width_, npix = w * height_;
    id.resize(npix);
    t.resize(npix);
    normal3.resize(3 * npix);
    albedo3.resize(3 * npix);
    const int n = (int)tiles_.size();
    if (n == 1) {
        if (cpt_read_gbuffer(tiles_[0].ctx, id.data(), t.data(), normal3.data(), albedo3.data(), npix) != CPT_OK)
            return Fail("cpt_read_gbuffer", tiles_[0].ctx);
        return true;
    }
    std::vector<int32_t> tid;
    std::vector<float> tt, tn, ta;
    for (int r = 0; r < n; ++r) {
        const std::vector<int32_t> rows = tile_rows(height_, n, r);
        const size_t m = rows.size() * w;
        tid.resize(m);
        tt.resize(m);
        tn.resize(3 * m);
        ta.resize(3 * m);
        if (cpt_read_gbuffer(tiles_[r].ctx, tid.data(), tt.data(), tn.data(), ta.data(), m) != CPT_OK)
            return Fail("cpt_read_gbuffer", tiles_[r].ctx);
        for (size_t k = 0; k < rows.size(); ++k) {
            const size_t dst = (size_t)rows[k] * w, src = k * w;
            std::copy(tid.begin() + src, tid.begin() + src + w, id.begin() + dst);
            std::copy(tt.begin() + src, tt.begin() + src + w, t.begin() + dst);
            std::copy(tn.begin() + 3 * src, tn.begin() + 3 * (src + w), normal3.begin() + 3 * dst);
            std::copy(ta.begin() + 3 * src, ta.begin() + 3 * (src + w), albedo3.begin() + 3 * dst);
        }
    }
    return true;
}

bool PathTracer::Reproject(const MotionalCamera& from, int max_history, float plane_tol) {
    if (!camera_) {
        err_ = "Reproject: SetCamera first";
        return false;
    }
    if (SceneBVH::BuildId() == 0) SceneBVH::BuildBVH();
    const MotionalCamera to = query_camera(*camera_), old = query_camera(from);
    std::lock_guard<std::mutex> lk(mu_);
    if (!SyncScene() || !EnsureFrame(to)) return false;
    if (frame_) {
        err_ = "Reproject: not available with SetDevices(n > 1), the row tiles own their accumulators";
        return false;
    }
    cpt_ctx* ctx = tiles_[0].ctx;
    if (cpt_reproject_accum(ctx, reinterpret_cast<const cpt_camera*>(&old), reinterpret_cast<const cpt_camera*>(&to), max_history,
                            plane_tol, ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u) != CPT_OK ||
        cpt_synchronize(ctx) != CPT_OK)
        return Fail("cpt_reproject_accum", ctx);
    NoteAccumCamera(to);
    NoteGBuffer(to);
    loop_history_ = false;   // the context's history is no longer the DispatchRay loop's
    return true;
}

bool PathTracer::CaptureHistory() {
    if (!camera_) {
        err_ = "CaptureHistory: SetCamera first";
        return false;
    }
    if (SceneBVH::BuildId() == 0) SceneBVH::BuildBVH();
    const MotionalCamera cam = query_camera(*camera_);
    std::lock_guard<std::mutex> lk(mu_);
    if (!SyncScene() || !EnsureFrame(cam)) return false;
    if (frame_) {
        err_ = "CaptureHistory: not available with SetDevices(n > 1), the row tiles own their accumulators";
        return false;
    }
    cpt_ctx* ctx = tiles_[0].ctx;
    gbuffer_known_ = false;
    if (cpt_history_capture(ctx, reinterpret_cast<const cpt_camera*>(&cam), ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u) != CPT_OK)
        return Fail("cpt_history_capture", ctx);
    NoteGBuffer(cam);
    loop_history_ = false;   // the context's history is no longer the DispatchRay loop's
    return true;
}

bool PathTracer::ReprojectTracked(int max_history, float plane_tol) {
    if (!camera_) {
        err_ = "ReprojectTracked: SetCamera first";
        return false;
    }
    const MotionalCamera to = query_camera(*camera_);
    std::lock_guard<std::mutex> lk(mu_);
    if (!SyncScene() || !EnsureFrame(to)) return false;   // the pending UpdateObjects are refit here
    if (frame_) {
        err_ = "ReprojectTracked: not available with SetDevices(n > 1), the row tiles own their accumulators";
        return false;
    }
    cpt_ctx* ctx = tiles_[0].ctx;
    if (cpt_reproject_accum_tracked(ctx, reinterpret_cast<const cpt_camera*>(&to), max_history, plane_tol,
                                    ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u) != CPT_OK ||
        cpt_synchronize(ctx) != CPT_OK)
        return Fail("cpt_reproject_accum_tracked", ctx);
    NoteAccumCamera(to);
    NoteGBuffer(to);
    loop_history_ = false;   // the context's history is no longer the DispatchRay loop's
    return true;
}

// Counters summed over the tiles (the render flags do not ask for CPT_RENDER_STATS, so these
// are the counters of the last counting render; GetStats after cpt-level counting renders).
bool PathTracer::GetStats(cpt_stats* out) {
    std::lock_guard<std::mutex> lk(mu_);
    if (tiles_.empty() || !out) return false;
    *out = cpt_stats{};
    for (Tile& t : tiles_) {
        cpt_stats s{};
        if (cpt_get_stats(t.ctx, &s) != CPT_OK) return Fail("cpt_get_stats", t.ctx);
        out->segments += s.segments;
        out->node_visits += s.node_visits;
        out->prim_tests += s.prim_tests;
        out->hits += s.hits;
        out->misses += s.misses;
    }
    return true;
}
