// cpt_api.cpp — PathTracer of the reference-shaped C++ construction API
// (include/cpppathtracer/path_tracer.h) on top of the C-ABI (include/cpt.h); the classes that never
// see a context are in cpt_api_scene.cpp.  Host code only; every GPU operation goes through cpt_*.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <algorithm>
#include <mutex>

#include "../../include/cpppathtracer/path_tracer.h"

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

static int address_mode_of(PocaAddressMode m) {
    switch (m) {
        case PocaAddressMode::Wrap: return CPT_ADDRESS_WRAP;
        case PocaAddressMode::Clamp: return CPT_ADDRESS_CLAMP;
        case PocaAddressMode::Border: return CPT_ADDRESS_BORDER;
        default: return CPT_ADDRESS_MIRROR;
    }
}

static const cpt_camera* as_cpt(const MotionalCamera& cam) { return reinterpret_cast<const cpt_camera*>(&cam); }

// The current camera with its basis computed, as GetCopy() gives it, but from a copy: the
// camera's own sample index (the display path's Mix weight) does not move for a query.
static MotionalCamera query_camera(const MotionalCamera& cam) {
    MotionalCamera c = cam;
    cpt_camera_get_copy(reinterpret_cast<cpt_camera*>(&c));
    return c;
}

// `cam` as FilterRadianceSpatial's records keep it: the basis computed, the sample index (which no
// first hit depends on) cleared, so that two copies of one camera compare equal byte for byte.
static MotionalCamera record_camera(const MotionalCamera& cam) {
    MotionalCamera c = query_camera(cam);
    c.cur_sample_idx_ = 0;
    return c;
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
            records_.accum_set = records_.gbuffer_known = false;   // a fresh frame: no radiance, no G-buffer
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

// The start of every public call that renders or traces at the current camera, in this order: the
// camera check; the BuildBVH the first such call owes (`build`; ReprojectTracked, which follows
// edits of an existing build, does not); the camera copy, taken outside mu_ (GetCopy takes the
// camera's mutex and advances the sample index, a query's copy does neither); mu_, which `lk` holds
// from here on; the scene and the frame brought to every context.
bool PathTracer::Begin(const char* who, CameraCopy how, bool build, MotionalCamera& cam, std::unique_lock<std::mutex>& lk) {
    if (!camera_) {
        err_ = std::string(who) + ": SetCamera first";
        return false;
    }
    if (build && SceneBVH::BuildId() == 0) SceneBVH::BuildBVH();
    cam = how == CameraCopy::Advance ? camera_->GetCopy() : query_camera(*camera_);
    lk = std::unique_lock<std::mutex>(mu_);
    return SyncScene() && EnsureFrame(cam);
}

bool PathTracer::RequireSingleDevice(const char* who, const char* owned) {
    if (!frame_) return true;
    err_ = std::string(who) + ": not available with SetDevices(n > 1), the row tiles own their " + owned;
    return false;
}

// A frame exists (and `and_also` holds), or LastError() is `msg`.
bool PathTracer::HaveFrame(const char* msg, bool and_also) {
    if (FrameCtx() && width_ != 0 && and_also) return true;
    err_ = msg;
    return false;
}

// The accumulator now belongs to `cam` (FilterRadianceSpatial).
void PathTracer::NoteAccumCamera(const MotionalCamera& cam) {
    records_.accum_cam = record_camera(cam);
    records_.accum_set = true;
}

// The first tile's frame G-buffer now holds `cam`'s first hits in the scene as that tile has it.
void PathTracer::NoteGBuffer(const MotionalCamera& cam) {
    records_.gbuffer_cam = record_camera(cam);
    records_.gbuffer_rev = tiles_[0].scene_rev;
    records_.gbuffer_known = true;
}

// The row tiles into the frame context: every gather queues behind its tile's render (events, no
// host wait); one wait at the end.
bool PathTracer::GatherTiles() {
    for (Tile& t : tiles_)
        if (cpt_gather_rows(frame_, t.ctx) != CPT_OK) return Fail("cpt_gather_rows", frame_);
    if (cpt_synchronize(frame_) != CPT_OK) return Fail("cpt_synchronize", frame_);
    for (Tile& t : tiles_)   // the tiles' device errors (their work is done by now)
        if (cpt_synchronize(t.ctx) != CPT_OK) return Fail("cpt_synchronize", t.ctx);
    return true;
}

// One render call, `launch(ctx, extra flags)`, named `what` to Fail: synchronous on the single
// context; with row tiles every tile's launch is queued first (each context's work runs on its own
// device and stream), then the tiles are gathered into the frame context.
template <class Launch>
bool PathTracer::LaunchOnTiles(const char* what, Launch launch) {
    if (!frame_) return launch(tiles_[0].ctx, (uint32_t)CPT_RENDER_SYNC) == CPT_OK || Fail(what, tiles_[0].ctx);
    for (Tile& t : tiles_)
        if (launch(t.ctx, 0u) != CPT_OK) return Fail(what, t.ctx);
    return GatherTiles();
}

// One render of `spp` passes at `cam`, the scene and the frame being on every context.
bool PathTracer::RenderPass(MotionalCamera& cam, int spp, bool accumulate) {
    NoteAccumCamera(cam);
    // heaviest tiles first (same image, shorter tail): many passes per pixel by a cost pilot, few (the
    // DispatchRay loop) by the previous pass's work, no pilot
    const uint32_t flags = CPT_RENDER_AUX | (accumulate ? CPT_RENDER_ACCUMULATE : 0u) | WalkFlags() |
                           (spp >= 64 ? CPT_SCHEDULE_COST : CPT_SCHEDULE_PREVIOUS);
    return LaunchOnTiles("cpt_render", [&](cpt_ctx* ctx, uint32_t extra) {
        return cpt_render(ctx, as_cpt(cam), spp, (int)max_recursion_depth_, flags | extra);
    });
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
            if (loop_.reproject) {
                ok = DisplayPassWithHistory(cma);
            } else {
                ok = SyncScene() && EnsureFrame(cma) && RenderPass(cma, 1, false);
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
    loop_.reproject = on;
    loop_.through_edits = on && through_edits;
    ForgetLoopHistory();   // whatever history the context holds is not this loop's
    loop_.max_history = max_history;
    loop_.plane_tol = plane_tol;
    loop_.prev_pass = false;   // the first pass after a switch restarts
    return true;
}

// (a frame under 16 pixels either way has no launch region: no display pass ever ran there)
bool PathTracer::PrevFits(bool had_prev) const {
    return had_prev && loop_.prev_cam.width_ == width_ && loop_.prev_cam.height_ == height_ && width_ >= 16 && height_ >= 16 &&
           !frame_;
}

// through_edits.  The context's captured history serves this loop only while it is the previous
// pass's: captured or renewed by this loop (loop_.history; Reproject, CaptureHistory,
// ReprojectTracked and SetDisplayReprojection clear it, the untracked C calls drop the capture
// itself), at the scene revision of the previous pass, and at a camera that equals prev_cam in
// every field but the sample index.  Anything else is not trusted: the history is captured anew
// at the previous pass's camera where the context still holds that pass's scene, and the display
// restarts where it does not.  False: cpt_history_info failed.
bool PathTracer::HistoryIsPrev(cpt_ctx* ctx, bool& is_prev) const {
    int valid = 0;
    cpt_camera cam;
    is_prev = false;
    if (cpt_history_info(ctx, &valid, &cam) != CPT_OK) return false;
    if (valid && loop_.history && loop_.history_rev == loop_.prev_rev) {
        cpt_camera prev = *as_cpt(loop_.prev_cam);
        prev.cur_sample_idx = cam.cur_sample_idx;
        is_prev = std::memcmp(&prev, &cam, sizeof(cam)) == 0;
    }
    return true;
}

// One pass of the loop with SetDisplayReprojection on (mu_ held): after a Refresh the display
// state moves to the new camera, or restarts where it cannot; then the pass and the per-pixel Mix.
// A pass that neither follows a Refresh nor a pass of this kind joins the mean the loop has so far
// through cpt_denoise_mix at the camera's index, which the per-pixel counts then continue from: the
// loop's first pass is such a one, its index being 2 after InitBuffers' copy (path_tracer.cu:258),
// so a still camera's frames are the reference loop's.
bool PathTracer::DisplayPassWithHistory(MotionalCamera& cma) {
    const bool had_prev = loop_.prev_pass, refreshed = cma.cur_sample_idx_ == 1;
    loop_.prev_pass = false;
    if (!had_prev) ForgetLoopHistory();
    return CaptureBeforeEdit(had_prev, refreshed) && SyncScene() && EnsureFrame(cma) && MoveDisplay(cma, had_prev, refreshed) &&
           PassAndMix(cma, !refreshed && !had_prev);
}

// A move or an edit is about to reach the context: capture before SyncScene lets it.  (Revision()
// is read before SyncScene reads it again: an UpdateObject from another thread that lands
// between the two is not seen here, no capture is made for it, and the pass below then finds an
// edited scene without a history of the previous pass and restarts the display.  Safe, but a
// restart that through_edits would otherwise have avoided.)
bool PathTracer::CaptureBeforeEdit(bool had_prev, bool refreshed) {
    if (loop_.through_edits && PrevFits(had_prev) && !tiles_.empty() && tiles_[0].scene_synced &&
        (refreshed || SceneBVH::Revision() != tiles_[0].scene_rev || tiles_[0].scene_rev != loop_.prev_rev)) {
        cpt_ctx* ctx = tiles_[0].ctx;
        bool is_prev = false;
        if (!HistoryIsPrev(ctx, is_prev)) return Fail("cpt_history_info", ctx);
        if (!is_prev) {
            ForgetLoopHistory();
            // (edits another call already brought to the context cannot be captured behind)
            if (tiles_[0].scene_build == loop_.prev_build && tiles_[0].scene_rev == loop_.prev_rev) {
                records_.gbuffer_known = false;   // the capture traces the frame's G-buffer
                if (cpt_history_capture(ctx, as_cpt(loop_.prev_cam), WalkFlags()) != CPT_OK) return Fail("cpt_history_capture", ctx);
                loop_.history = true;
                loop_.history_rev = loop_.prev_rev;
            }
        }
    }
    return true;
}

// After a Refresh or (through_edits) an edit of the same build, the scene being on the context: the
// display state moves to `cma`, or restarts where it cannot.
bool PathTracer::MoveDisplay(const MotionalCamera& cma, bool had_prev, bool refreshed) {
    const Tile& t0 = tiles_[0];
    const bool same_build = t0.scene_build == loop_.prev_build, same_rev = t0.scene_rev == loop_.prev_rev;
    const bool edited = loop_.through_edits && had_prev && same_build && !same_rev;
    if (!refreshed && !edited) return true;
    bool carry = PrevFits(had_prev) && same_build && (same_rev || loop_.through_edits);
    if (carry && loop_.through_edits) {
        // dropped by a new frame or scene, never captured, or not the previous pass's: restart
        if (!HistoryIsPrev(t0.ctx, carry)) return Fail("cpt_history_info", t0.ctx);
    }
    if (carry) records_.gbuffer_known = false;   // both reprojection calls trace the frame's G-buffer
    if (carry && loop_.through_edits) {
        if (cpt_reproject_display_tracked(t0.ctx, as_cpt(cma), loop_.max_history, loop_.plane_tol, WalkFlags()) != CPT_OK)
            return Fail("cpt_reproject_display_tracked", t0.ctx);
        loop_.history_rev = t0.scene_rev;   // the call renewed the history: cma, the current objects
    } else if (carry) {
        if (cpt_reproject_display(t0.ctx, as_cpt(loop_.prev_cam), as_cpt(cma), loop_.max_history, loop_.plane_tol, WalkFlags()) !=
            CPT_OK)
            return Fail("cpt_reproject_display", t0.ctx);
    } else {
        ForgetLoopHistory();
        if (cpt_reset_display(FrameCtx()) != CPT_OK) return Fail("cpt_reset_display");
    }
    return true;
}

// The pass (with the sync every pass of the loop starts with: an edit that landed since the one
// above reaches the context here), the Mix, joining the loop's mean so far at the camera's index
// (`join_mean`) or per pixel, and the record of this pass for the next.
bool PathTracer::PassAndMix(MotionalCamera& cma, bool join_mean) {
    if (!SyncScene() || !EnsureFrame(cma) || !RenderPass(cma, 1, false)) return false;
    if (join_mean) {
        if (cpt_denoise_mix(FrameCtx(), cma.cur_sample_idx_, output_buffer_.data()) != CPT_OK) return Fail("cpt_denoise_mix");
    } else if (cpt_denoise_mix_history(FrameCtx(), output_buffer_.data()) != CPT_OK) {
        return Fail("cpt_denoise_mix_history");
    }
    loop_.prev_cam = cma;
    loop_.prev_build = tiles_[0].scene_build;
    loop_.prev_rev = tiles_[0].scene_rev;
    loop_.prev_pass = true;
    return true;
}

void PathTracer::Stop() {
    if (!running_.exchange(false)) return;
    cv_.notify_all();
    if (worker_.joinable()) worker_.join();
}

bool PathTracer::Render(int spp, bool accumulate) {
    MotionalCamera cam;
    std::unique_lock<std::mutex> lk;
    return Begin("Render", CameraCopy::Advance, true, cam, lk) && RenderPass(cam, spp, accumulate);
}

// Top-up render (cpt_render_to_count): as RenderPass, every row tile on its own
// accumulator, then the gather.
bool PathTracer::RenderToCount(int target) {
    MotionalCamera cam;
    std::unique_lock<std::mutex> lk;
    if (!Begin("RenderToCount", CameraCopy::Advance, true, cam, lk)) return false;
    NoteAccumCamera(cam);
    const uint32_t flags = CPT_RENDER_AUX | WalkFlags();
    return LaunchOnTiles("cpt_render_to_count", [&](cpt_ctx* ctx, uint32_t extra) {
        return cpt_render_to_count(ctx, as_cpt(cam), target, (int)max_recursion_depth_, flags | extra);
    });
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
        if (cpt_adaptive_begin(tiles_[i].ctx, as_cpt(cam), min_spp, max_spp, batch, rel_error, (int)max_recursion_depth_, flags) !=
            CPT_OK)
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
    if (!GatherTiles()) return false;
    int most = 0;
    uint64_t sum = 0;
    for (Tile& t : tiles_) {   // (each tile synchronised by the gather)
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
    MotionalCamera cma;
    std::unique_lock<std::mutex> lk;
    if (!Begin("RenderAdaptive", CameraCopy::Advance, true, cma, lk)) return false;
    NoteAccumCamera(cma);   // for the row tiles too (RenderAdaptiveTiles)
    const uint32_t flags = CPT_RENDER_AUX | WalkFlags() | (max_spp >= 64 ? CPT_SCHEDULE_COST : 0u);
    if (frame_) return RenderAdaptiveTiles(cma, min_spp, max_spp, batch, rel_error, flags, rounds, passes_done);
    cpt_ctx* ctx = tiles_[0].ctx;
    if (cpt_render_adaptive(ctx, as_cpt(cma), min_spp, max_spp, batch, rel_error, (int)max_recursion_depth_, flags) != CPT_OK)
        return Fail("cpt_render_adaptive", ctx);
    if (cpt_adaptive_info(ctx, rounds, nullptr, 0, passes_done) != CPT_OK) return Fail("cpt_adaptive_info", ctx);
    return true;
}

bool PathTracer::ReadNoise(float* rel) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!HaveFrame("ReadNoise: RenderAdaptive first")) return false;
    if (cpt_read_noise(FrameCtx(), rel, (size_t)width_ * height_) != CPT_OK) return Fail("cpt_read_noise");
    return true;
}

bool PathTracer::FilterRadiance(int levels, float sigma_l, int sharpness) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!HaveFrame("FilterRadiance: RenderAdaptive first")) return false;
    if (cpt_filter_frame(FrameCtx(), levels, sigma_l, sharpness) != CPT_OK) return Fail("cpt_filter_frame");
    return true;
}

bool PathTracer::FilterRadianceSpatial(int levels, float sigma_l, int sharpness) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!HaveFrame("FilterRadianceSpatial: Render first", records_.accum_set)) return false;
    if (!RequireSingleDevice("FilterRadianceSpatial", "G-buffers")) return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    // the G-buffer the context holds is reused only if it is the accumulator's camera's, in the
    // scene the context has now
    if (!records_.gbuffer_known || records_.gbuffer_rev != tiles_[0].scene_rev ||
        std::memcmp(&records_.gbuffer_cam, &records_.accum_cam, sizeof(records_.accum_cam)) != 0) {
        records_.gbuffer_known = false;
        if (cpt_gbuffer(ctx, as_cpt(records_.accum_cam), WalkFlags()) != CPT_OK) return Fail("cpt_gbuffer", ctx);
        NoteGBuffer(records_.accum_cam);
    }
    if (cpt_filter_frame_spatial(ctx, levels, sigma_l, sharpness) != CPT_OK) return Fail("cpt_filter_frame_spatial", ctx);
    return true;
}

bool PathTracer::ReadFiltered(std::vector<float>& rgb) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!HaveFrame("ReadFiltered: FilterRadiance first")) return false;
    rgb.resize((size_t)width_ * height_ * 3);
    if (cpt_read_filtered(FrameCtx(), rgb.data(), nullptr, (size_t)width_ * height_) != CPT_OK)
        return Fail("cpt_read_filtered");
    return true;
}

bool PathTracer::ReadRadiance(std::vector<float>& rgb) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!HaveFrame("ReadRadiance: nothing rendered")) return false;
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

// `rgb` as a PFM file; where it cannot be written, `err` is `who`'s message.
static bool write_pfm(const char* who, const std::string& path, const std::vector<float>& rgb, int width, int height,
                      std::string& err) {
    std::ofstream f(path, std::ios::binary);
    if (f) {
        f << "PF\n" << width << " " << height << "\n-1.0\n";
        for (int y = height - 1; y >= 0; --y)   // PFM rows are bottom-to-top
            f.write(reinterpret_cast<const char*>(&rgb[(size_t)y * width * 3]), (std::streamsize)width * 3 * sizeof(float));
        if (f) return true;
    }
    err = std::string(who) + ": cannot write " + path;
    return false;
}

bool PathTracer::SaveRadiancePFM(const std::string& path) {
    std::vector<float> rgb;
    return ReadRadiance(rgb) && write_pfm("SaveRadiancePFM", path, rgb, width_, height_, err_);
}

bool PathTracer::SaveFilteredPFM(const std::string& path) {
    std::vector<float> rgb;
    return ReadFiltered(rgb) && write_pfm("SaveFilteredPFM", path, rgb, width_, height_, err_);
}

int PathTracer::Pick(int x, int y, float* t) {
    MotionalCamera cma;
    std::unique_lock<std::mutex> lk;
    if (!Begin("Pick", CameraCopy::Query, true, cma, lk)) return -1;
    int32_t object = -1;
    if (cpt_pick(tiles_[0].ctx, as_cpt(cma), x, y, WalkFlags(), &object, t) != CPT_OK) {
        Fail("cpt_pick", tiles_[0].ctx);
        return -1;
    }
    return object;
}

// Every tile's G-buffer is queued first, then each is read into its rows of the frame.
bool PathTracer::ReadGBuffer(std::vector<int32_t>& id, std::vector<float>& t, std::vector<float>& normal3,
                             std::vector<float>& albedo3) {
    MotionalCamera cma;
    std::unique_lock<std::mutex> lk;
    if (!Begin("ReadGBuffer", CameraCopy::Query, true, cma, lk)) return false;
    records_.gbuffer_known = false;
    for (Tile& tile : tiles_)
        if (cpt_gbuffer(tile.ctx, as_cpt(cma), WalkFlags()) != CPT_OK) return Fail("cpt_gbuffer", tile.ctx);
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
        // the tile's k-th row of a plane of `c` components per pixel to the frame's row rows[k]
        auto scatter = [&](const auto& tile_plane, auto& plane, size_t c) {
            for (size_t k = 0; k < rows.size(); ++k)
                std::copy(tile_plane.begin() + c * k * w, tile_plane.begin() + c * (k + 1) * w, plane.begin() + c * rows[k] * w);
        };
        scatter(tid, id, 1);
        scatter(tt, t, 1);
        scatter(tn, normal3, 3);
        scatter(ta, albedo3, 3);
    }
    return true;
}

bool PathTracer::Reproject(const MotionalCamera& from, int max_history, float plane_tol) {
    const MotionalCamera old = query_camera(from);
    MotionalCamera to;
    std::unique_lock<std::mutex> lk;
    if (!Begin("Reproject", CameraCopy::Query, true, to, lk) || !RequireSingleDevice("Reproject", "accumulators")) return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    if (cpt_reproject_accum(ctx, as_cpt(old), as_cpt(to), max_history, plane_tol, WalkFlags()) != CPT_OK ||
        cpt_synchronize(ctx) != CPT_OK)
        return Fail("cpt_reproject_accum", ctx);
    NoteAccumCamera(to);
    NoteGBuffer(to);
    ForgetLoopHistory();
    return true;
}

bool PathTracer::CaptureHistory() {
    MotionalCamera cam;
    std::unique_lock<std::mutex> lk;
    if (!Begin("CaptureHistory", CameraCopy::Query, true, cam, lk) || !RequireSingleDevice("CaptureHistory", "accumulators"))
        return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    records_.gbuffer_known = false;
    if (cpt_history_capture(ctx, as_cpt(cam), WalkFlags()) != CPT_OK) return Fail("cpt_history_capture", ctx);
    NoteGBuffer(cam);
    ForgetLoopHistory();
    return true;
}

bool PathTracer::ReprojectTracked(int max_history, float plane_tol) {
    MotionalCamera to;
    std::unique_lock<std::mutex> lk;
    // (no BuildBVH; the pending UpdateObjects are refit by Begin's sync)
    if (!Begin("ReprojectTracked", CameraCopy::Query, false, to, lk) || !RequireSingleDevice("ReprojectTracked", "accumulators"))
        return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    if (cpt_reproject_accum_tracked(ctx, as_cpt(to), max_history, plane_tol, WalkFlags()) != CPT_OK ||
        cpt_synchronize(ctx) != CPT_OK)
        return Fail("cpt_reproject_accum_tracked", ctx);
    NoteAccumCamera(to);
    NoteGBuffer(to);
    ForgetLoopHistory();
    return true;
}

// Presenting: the three calls start as every call at the current camera does and
// need the one context that owns the accumulator and the filter planes.
bool PathTracer::SetExposure(float exposure) {
    MotionalCamera cam;
    std::unique_lock<std::mutex> lk;
    if (!Begin("SetExposure", CameraCopy::Query, true, cam, lk) || !RequireSingleDevice("SetExposure", "accumulators")) return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    return cpt_set_exposure(ctx, exposure) == CPT_OK || Fail("cpt_set_exposure", ctx);
}

bool PathTracer::MeterExposure(bool filtered, float key, int permille, float adapt) {
    MotionalCamera cam;
    std::unique_lock<std::mutex> lk;
    if (!Begin("MeterExposure", CameraCopy::Query, true, cam, lk) || !RequireSingleDevice("MeterExposure", "accumulators"))
        return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    return cpt_meter_exposure(ctx, filtered ? CPT_PRESENT_FILTERED : CPT_PRESENT_ACCUM, key, permille, adapt) == CPT_OK ||
           Fail("cpt_meter_exposure", ctx);
}

bool PathTracer::Present(std::vector<uint8_t>& bgra, int tone, bool srgb, bool filtered, float white) {
    MotionalCamera cam;
    std::unique_lock<std::mutex> lk;
    if (!Begin("Present", CameraCopy::Query, true, cam, lk) || !RequireSingleDevice("Present", "accumulators")) return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    if (cpt_present(ctx, filtered ? CPT_PRESENT_FILTERED : CPT_PRESENT_ACCUM, tone, white, srgb ? CPT_TRANSFER_SRGB : CPT_TRANSFER_LINEAR,
                    nullptr) != CPT_OK)
        return Fail("cpt_present", ctx);
    bgra.resize((size_t)width_ * height_ * 4);
    return cpt_read_present(ctx, bgra.data(), bgra.size()) == CPT_OK || Fail("cpt_read_present", ctx);
}

// Antialiased presentation: as the presenting calls above.  ResolveCoverage leaves
// the context's G-buffer at the current camera, which it records as ReadGBuffer does.
bool PathTracer::ResolveCoverage(int samples, float normal_cos) {
    MotionalCamera cam;
    std::unique_lock<std::mutex> lk;
    if (!Begin("ResolveCoverage", CameraCopy::Query, true, cam, lk) || !RequireSingleDevice("ResolveCoverage", "G-buffers")) return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    records_.gbuffer_known = false;
    if (cpt_aa_coverage(ctx, as_cpt(cam), WalkFlags(), samples, normal_cos) != CPT_OK) return Fail("cpt_aa_coverage", ctx);
    NoteGBuffer(cam);
    return true;
}

bool PathTracer::PresentAntialiased(std::vector<uint8_t>& bgra, int tone, bool srgb, bool filtered, float white) {
    MotionalCamera cam;
    std::unique_lock<std::mutex> lk;
    if (!Begin("PresentAntialiased", CameraCopy::Query, true, cam, lk) || !RequireSingleDevice("PresentAntialiased", "accumulators"))
        return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    if (cpt_present_aa(ctx, filtered ? CPT_PRESENT_FILTERED : CPT_PRESENT_ACCUM, tone, white, srgb ? CPT_TRANSFER_SRGB : CPT_TRANSFER_LINEAR,
                       nullptr) != CPT_OK)
        return Fail("cpt_present_aa", ctx);
    bgra.resize((size_t)width_ * height_ * 4);
    return cpt_read_present(ctx, bgra.data(), bgra.size()) == CPT_OK || Fail("cpt_read_present", ctx);
}

// Bloom: as the presenting calls above.
bool PathTracer::BuildBloom(bool filtered, float threshold, int levels) {
    MotionalCamera cam;
    std::unique_lock<std::mutex> lk;
    if (!Begin("BuildBloom", CameraCopy::Query, true, cam, lk) || !RequireSingleDevice("BuildBloom", "accumulators")) return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    return cpt_bloom(ctx, filtered ? CPT_PRESENT_FILTERED : CPT_PRESENT_ACCUM, threshold, levels) == CPT_OK || Fail("cpt_bloom", ctx);
}

bool PathTracer::PresentBloom(std::vector<uint8_t>& bgra, int tone, bool srgb, bool filtered, float white, float intensity) {
    MotionalCamera cam;
    std::unique_lock<std::mutex> lk;
    if (!Begin("PresentBloom", CameraCopy::Query, true, cam, lk) || !RequireSingleDevice("PresentBloom", "accumulators")) return false;
    cpt_ctx* ctx = tiles_[0].ctx;
    if (cpt_present_bloom(ctx, filtered ? CPT_PRESENT_FILTERED : CPT_PRESENT_ACCUM, tone, white, srgb ? CPT_TRANSFER_SRGB : CPT_TRANSFER_LINEAR,
                          intensity, nullptr) != CPT_OK)
        return Fail("cpt_present_bloom", ctx);
    bgra.resize((size_t)width_ * height_ * 4);
    return cpt_read_present(ctx, bgra.data(), bgra.size()) == CPT_OK || Fail("cpt_read_present", ctx);
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
