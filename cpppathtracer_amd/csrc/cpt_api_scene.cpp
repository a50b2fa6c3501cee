// cpt_api_scene.cpp — the part of the reference-shaped C++ API (include/cpppathtracer/*.h) that
// never sees a context: Object, MotionalCamera, the SceneBVH statics and PocaTextureUtils.  Host
// code only; PathTracer (cpt_api.cpp) brings their state to the GPU through cpt_*.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <set>

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
