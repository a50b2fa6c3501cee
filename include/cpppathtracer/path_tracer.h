// path_tracer.h — PathTracer, the drop-in surface of the reference's hot path
// (reference include/path_tracer.h:15-50, cuSrc/path_tracer.cu).
//
// Reference interface, same names and meaning:
//   AddObject(Object*)            register an object (path_tracer.cu:29-34)
//   InitPipeline()                build the BVH, start the render thread (:308-314)
//   DispatchRay(DispatchRayArgs)  queue one pass; the render thread runs SamplePixel for one
//                                 sample per pixel, the 5x5 denoise and the running-mean Mix,
//                                 then calls Callback(BGRA8, width, height, cbParam) (:256-306)
//   SetCamera / GetCamera
// Additions the headless configs need (the reference has no setters for these):
//   SetMaxRecursionDepth, SetSeed, SetDevice, SetDevices (row tiling over several GPUs),
//   SetEnvTexture, Render(spp) (synchronous), RenderAdaptive, ReadNoise, FilterRadiance, FilterRadianceSpatial,
//   ReadFiltered, SaveFilteredPFM, ReadRadiance, ReadFrameBGRA, SaveRadiancePFM, Pick, ReadGBuffer,
//   Reproject, CaptureHistory, ReprojectTracked, RenderToCount, SetDisplayReprojection, SetExposure,
//   MeterExposure, Present, ResolveCoverage, PresentAntialiased, BuildBloom, PresentBloom, GetStats, Stop.
// Errors: the reference logs CUDA errors and continues; here every call that reaches the
// GPU returns false on failure and LastError() holds the message (no exceptions).
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bvh.h"
#include "motional_camera.h"
#include "object.h"
#include "ray_tracing_common.h"
#include "textures.h"

#define MAX_RECURSION_DEPTH_SET 32

class PathTracer {
public:
    PathTracer();
    ~PathTracer();

    void AddObject(Object* obj);
    void InitPipeline();
    void DispatchRay(DispatchRayArgs args);
    void SetCamera(std::shared_ptr<MotionalCamera>& camera);
    std::shared_ptr<MotionalCamera> GetCamera();

    // ---- additions ------------------------------------------------------------------
    bool SetMaxRecursionDepth(uint depth);      // 0..32; reference default 8 (path_tracer.h:43)
    void SetSeed(uint64_t seed);                // reference seeds with clock() (path_tracer.cu:107)
    bool SetDevice(int device);                 // before the first render
    // Row tiling, before the first render: the image rows are dealt to n
    // contexts in interleaved 8-row blocks, one context per device (device i % visible devices,
    // or the listed devices; a device may repeat), each rendering its rows of every pass.  Each
    // pass's tiles are gathered into one frame on the first device (peer copies + a stitch
    // kernel, cpt_gather_rows), which ReadRadiance, ReadFrameBGRA and the DispatchRay display
    // path read.  A pixel's stream depends only on (seed, x, y): the image is bit-identical to
    // a single-device render.
    bool SetDevices(int n);
    bool SetDevices(const std::vector<int>& devices);
    int DeviceCount() const { return (int)std::max<size_t>(1, device_list_.size()); }
    bool SetEnvTexture(PocaTexture tex);        // default: textures/sky (assets/sky.cptex)
    // BVH walk: true (default) = CPT_TRAVERSAL_ORDERED (same image, fewer node visits);
    // false = the reference's right-first DFS order (its node/prim counts in GetStats).
    void SetOrderedTraversal(bool on) { ordered_walk_ = on; }
    // Synchronous `spp` passes into the radiance accumulator (accumulate=false restarts it).
    bool Render(int spp, bool accumulate = true);
    // Synchronous adaptive render into a restarted accumulator (cpt_render_adaptive): rounds of
    // `batch` passes over the 8x8 tiles whose pixels have not all reached a relative standard
    // error of rel_error; none stops before min_spp, all at max_spp.  Each pixel ends as a
    // Render of its own pass count would leave it.  With SetDevices every tile's rounds are queued
    // on its own device and stepped in turn from this thread (cpt_adaptive_begin / _step), then
    // the tiles and their moments are gathered: the frame, the noise map and the filter's result
    // are those of one device, bit for bit.  rounds / passes_done (optional): the rounds run (the
    // most of any tile) and the pixel passes of all of them (summed over the tiles).
    bool RenderAdaptive(int min_spp, int max_spp, int batch, float rel_error, int* rounds = nullptr,
                        uint64_t* passes_done = nullptr);
    // The last RenderAdaptive's per-pixel relative standard error, float[width*height].
    bool ReadNoise(float* rel);
    // Variance-guided a-trous filter of the last RenderAdaptive's frame (cpt_filter_frame):
    // `levels` 5x5 iterations (0..8) at step 1, 2, 4, ..., edge-stopped by the first-hit normals
    // (max(N.N', 0) squared `sharpness` times, 0..10) and by luminance differences of more than
    // about sigma_l standard errors of the pixel's mean.  The radiance accumulator is not
    // changed; ReadFiltered / SaveFilteredPFM read the result (rgb float[width*height*3]).
    bool FilterRadiance(int levels = 5, float sigma_l = 1.0f, int sharpness = 7);
    // The same filter for a frame without moments: what Render, Reproject / ReprojectTracked and
    // RenderToCount leave (cpt_filter_frame_spatial).  The variance comes from each
    // pixel's 7x7 window and the levels are guided by the G-buffer of the camera the radiance
    // belongs to, the one of the last Render / RenderAdaptive / RenderToCount / Reproject*.  A
    // reprojection leaves that G-buffer; where the context holds another (none yet, one that
    // ReadGBuffer or CaptureHistory traced at a camera moved since, one of the scene before an
    // edit) it is traced here first, so the current camera may look elsewhere meanwhile.
    // ReadFiltered / SaveFilteredPFM read the result.  Not available with SetDevices(n > 1)
    // (false, LastError).
    bool FilterRadianceSpatial(int levels = 3, float sigma_l = 2.0f, int sharpness = 3);
    bool ReadFiltered(std::vector<float>& rgb);
    bool SaveFilteredPFM(const std::string& path);
    // Per-pixel mean radiance, rgb float[width*height*3] (row-major, y down).
    bool ReadRadiance(std::vector<float>& rgb);
    // Last display frame (denoised running mean), BGRA8[width*height*4].
    bool ReadFrameBGRA(std::vector<uint8_t>& bgra);
    bool SaveRadiancePFM(const std::string& path);
    // The object under pixel (x, y) of the current camera's image (cpt_pick): its AddObject index,
    // or -1 for the sky, a pixel outside the image or a failure (LastError() then holds the
    // message); *t, when given, gets the hit distance (1e30 on a miss).  The ray is the pixel's
    // centre ray (no lens sample); pending UpdateObjects are refit first, as Render does.  With
    // SetDevices the ray runs on the first tile's context.  The camera's sample index, the
    // accumulator and the RNG are left as they are.
    int Pick(int x, int y, float* t = nullptr);
    // The G-buffer of the current camera's full frame (cpt_gbuffer, row-major, y down): object
    // index (-1: sky), hit distance, normal and albedo (float[width*height*3] each) per pixel.
    bool ReadGBuffer(std::vector<int32_t>& id, std::vector<float>& t, std::vector<float>& normal3,
                     std::vector<float>& albedo3);
    // Keeps the accumulated radiance through a camera move (cpt_reproject_accum): the accumulator,
    // rendered with `from` (a copy of the camera object the caller kept from its last Render), is
    // looked up at the current camera, so the next Render(spp, true) adds to the history instead
    // of restarting it.  A pixel keeps at most max_history passes; a history pixel counts only
    // where it saw the same object within plane_tol x the hit distance of the new hit's tangent
    // plane; pixels without history restart.  Static scene only (after UpdateObject, restart with
    // Render(spp, false)); mirrors and glass lag until new passes outweigh the history.  The
    // current camera's sample index, the RNG and the display state are left as they are; the
    // DispatchRay loop (the Mix running mean with its one global sample index) does not use it.
    // Not available with SetDevices(n > 1): the row tiles own their accumulators (false, LastError).
    bool Reproject(const MotionalCamera& from, int max_history = 32, float plane_tol = 1e-2f);
    // Keeps the DispatchRay loop's running mean through camera moves (cpt_reproject_display,
    // cpt_denoise_mix_history).  Off (the default): the loop is the reference's, Mix at
    // 1 / cur_sample_idx (path_tracer.cu:241-254, 256-306), a raw one-sample frame after every
    // MotionalCamera::Refresh.  On: every pass displays with the per-pixel Mix, and a pass whose
    // camera copy has cur_sample_idx_ == 1 (a Refresh happened) first looks the previous pass's mean
    // and sample counts up at the new camera, provided the previous pass's camera had the frame's
    // size and the scene has not been edited or rebuilt since that pass; otherwise the display
    // restarts from zero.  The first pass after this call, unless it follows a Refresh, is mixed at
    // the camera's index as the reference's is, and the per-pixel counts continue from that index:
    // a still camera gives the reference's running mean, bit for bit.  max_history and plane_tol as
    // Reproject's; max_history < 1 or a negative or non-finite plane_tol changes nothing (false,
    // LastError).  A frame narrower or lower than 16 pixels has no display launch region: its loop
    // delivers zero frames, on or off.  With SetDevices(n > 1) the frame context holds no scene to
    // trace, so every Refresh restarts.
    // through_edits (off by default: the loop above, byte for byte): a pass that follows a Refresh
    // or a changed SceneBVH revision of the same build moves the display state with
    // cpt_reproject_display_tracked, which follows edited objects (UpdateObject) back to where the
    // history saw them; the first such pass captures the history at the previous pass's camera,
    // before the edits reach the context, and the loop uses no history but one it captured or
    // renewed itself (Reproject, CaptureHistory, ReprojectTracked between passes make the next move
    // capture again; edits that another call already brought to the context restart the display).
    // A new BuildBVH still restarts.
    bool SetDisplayReprojection(bool on, int max_history = 32, float plane_tol = 1e-2f, bool through_edits = false);
    // Reproject through object edits (cpt_history_capture, cpt_reproject_accum_tracked; DESIGN.md
    // §23).  CaptureHistory(): after a Render, before moving the camera or editing objects: keeps
    // the current camera's G-buffer and the objects as they are.  ReprojectTracked(): after
    // UpdateObject calls and / or a camera move: the accumulator is looked up at the current camera
    // with every hit followed back to where its object stood at the capture (an object whose type
    // or material changed restarts); the current camera and objects become the captured history,
    // so the cycle edit, ReprojectTracked, Render(spp, true) repeats without another capture.
    // Shadows and reflections of moved objects lag as mirrors do in Reproject.  Both return false
    // with SetDevices(n > 1), as Reproject does.
    bool CaptureHistory();
    // Top-up render (cpt_render_to_count; an addition: the reference gives every
    // pixel the same passes): every pixel runs the passes its accumulator count lacks to `target`
    // (1 .. 2^20), as a Render(d, true) of its own deficit d would; pixels at or past the target
    // are left untouched.  After Reproject / ReprojectTracked it spends the passes on the
    // disoccluded pixels.  Synchronous.  With SetDevices(n > 1) it runs on every row tile and
    // gathers, as Render does.
    bool RenderToCount(int target);
    bool ReprojectTracked(int max_history = 32, float plane_tol = 1e-2f);
    // Presenting the HDR frame (cpt_set_exposure, cpt_meter_exposure, cpt_present; an
    // addition: the DispatchRay loop clamps its own running mean to [0, 1]).  Present: the radiance
    // accumulator, or with `filtered` the last FilterRadiance / FilterRadianceSpatial result, times
    // the exposure, through the tone curve (CPT_TONE_CLAMP, CPT_TONE_REINHARD with `white` > 0,
    // CPT_TONE_ACES) and the sRGB transfer (`srgb` false: the reference's 255.99 * linear) into
    // BGRA8[width*height*4].  MeterExposure moves the exposure towards key / (the permille-th
    // thousandth of the frame's positive luminances, to an eighth of an octave) by the share `adapt`
    // in [0, 1]; SetExposure sets it (finite, > 0; 1 on a new frame).  The radiance, the RNG, the
    // filter result and the display loop's state are left as they are.  Not available with
    // SetDevices(n > 1) (false, LastError).
    bool SetExposure(float exposure);
    bool MeterExposure(bool filtered = false, float key = 0.18f, int permille = 500, float adapt = 1.0f);
    bool Present(std::vector<uint8_t>& bgra, int tone = CPT_TONE_ACES, bool srgb = true, bool filtered = false, float white = 4.0f);
    // Antialiased presentation (cpt_aa_coverage, cpt_present_aa; an addition: RayGen
    // shoots every pass of a pixel through the same point of it).  ResolveCoverage traces samples x
    // samples (2 or 4) first-hit rays inside every pixel on a geometric edge at the current camera
    // (an id change among its 8 neighbours, or a normal turned past normal_cos) and attributes them
    // to the neighbours whose centre saw the same surface; it leaves the G-buffer at that camera.
    // PresentAntialiased is Present with every pixel the coverage-weighted mix of those neighbours'
    // tone-mapped colours; it needs a ResolveCoverage since the frame was made, and a new one after
    // a camera move or an object edit.  Not available with SetDevices(n > 1) (false, LastError).
    bool ResolveCoverage(int samples = 4, float normal_cos = 0.9f);
    bool PresentAntialiased(std::vector<uint8_t>& bgra, int tone = CPT_TONE_ACES, bool srgb = true, bool filtered = false,
                            float white = 4.0f);
    // Bloom (cpt_bloom, cpt_present_bloom; an addition).  BuildBloom makes the pyramid
    // of the light above `threshold` (in exposed units, so after SetExposure / MeterExposure) of the
    // radiance accumulator, or with `filtered` of the last filter result, over `levels` (1..8) halvings.
    // PresentBloom is Present with `intensity` (finite, >= 0) times the pyramid's sum added to every
    // pixel in front of the tone curve; it needs a BuildBloom since the frame was made.  Not available
    // with SetDevices(n > 1) (false, LastError).
    bool BuildBloom(bool filtered = false, float threshold = 1.0f, int levels = 6);
    bool PresentBloom(std::vector<uint8_t>& bgra, int tone = CPT_TONE_ACES, bool srgb = true, bool filtered = false, float white = 4.0f,
                      float intensity = 0.25f);
    bool GetStats(cpt_stats* out);
    void Stop();                                 // stop the render thread (also in ~PathTracer)
    const std::string& LastError() const { return err_; }

private:
    // One libcpt context: the renderer of one row tile (or of the whole frame).
    struct Tile {
        cpt_ctx* ctx = nullptr;
        int device = 0;
        bool scene_synced = false;
        uint64_t scene_build = 0;      // SceneBVH::BuildId() uploaded to the context
        uint64_t scene_rev = 0;        // SceneBVH::Revision() the context is at
        std::vector<uint64_t> updates_seen;     // per-object UpdateObject counts refit so far
        std::vector<uint64_t> bound_textures;   // material texture handles bound on the context
        bool env_uploaded = false;
        bool rng_ready = false;
    };
    // One read of SceneBVH's state (SceneBVH::GetState), applied to every tile of a pass, so all
    // row tiles of a frame render the same scene revision.
    struct SceneSnap {
        uint64_t build = 0, rev = 0;
        std::vector<cpt_object> built, current;
        std::vector<uint64_t> updates;
    };
    // FilterRadianceSpatial compares two records.  The camera the radiance belongs to: every
    // call that renders into or reprojects the accumulator notes it (NoteAccumCamera).  And what the
    // first tile's frame G-buffer holds, a camera in a scene revision: every call that writes that
    // G-buffer notes it (NoteGBuffer) or, where it is not worth following, forgets it
    // (gbuffer_known = false), as a new frame does.
    struct FrameRecords {
        bool accum_set = false, gbuffer_known = false;
        MotionalCamera accum_cam, gbuffer_cam;
        uint64_t gbuffer_rev = 0;
    } records_;
    // The DispatchRay loop's display state: SetDisplayReprojection's settings, and the previous pass
    // of the loop, its camera copy and scene state.
    struct DisplayLoop {
        bool reproject = false, through_edits = false;
        int max_history = 32;
        float plane_tol = 1e-2f;
        bool prev_pass = false;
        MotionalCamera prev_cam;
        uint64_t prev_build = 0, prev_rev = 0;
        // through_edits: the context's captured history was captured or renewed by the loop, for the
        // scene revision history_rev
        bool history = false;
        uint64_t history_rev = 0;
    } loop_;
    enum class CameraCopy { Advance, Query };   // GetCopy() (the renders) or a copy that leaves the sample index
    bool EnsureContext();
    bool SyncScene();
    bool SyncTile(Tile& t, const SceneSnap& snap);
    bool BindTextures(Tile& t, const std::vector<cpt_object>& objs);
    bool EnsureFrame(const MotionalCamera& cam);
    bool Begin(const char* who, CameraCopy how, bool build, MotionalCamera& cam, std::unique_lock<std::mutex>& lk);
    bool RequireSingleDevice(const char* who, const char* owned);
    bool HaveFrame(const char* msg, bool and_also = true);
    template <class Launch> bool LaunchOnTiles(const char* what, Launch launch);
    bool GatherTiles();
    bool RenderPass(MotionalCamera& cam, int spp, bool accumulate);
    bool RenderAdaptiveTiles(MotionalCamera& cam, int min_spp, int max_spp, int batch, float rel_error, uint32_t flags,
                             int* rounds, uint64_t* passes_done);
    bool DisplayPassWithHistory(MotionalCamera& cam);
    bool CaptureBeforeEdit(bool had_prev, bool refreshed);
    bool MoveDisplay(const MotionalCamera& cam, bool had_prev, bool refreshed);
    bool PassAndMix(MotionalCamera& cam, bool join_mean);
    bool PrevFits(bool had_prev) const;
    bool HistoryIsPrev(cpt_ctx* ctx, bool& is_prev) const;
    void ForgetLoopHistory() { loop_.history = false; }   // the context's history is not (or no longer) the loop's
    void NoteAccumCamera(const MotionalCamera& cam);
    void NoteGBuffer(const MotionalCamera& cam);
    void PipelineLoop();
    bool Fail(const char* what, cpt_ctx* ctx = nullptr);
    cpt_ctx* FrameCtx() const { return frame_ ? frame_ : (tiles_.empty() ? nullptr : tiles_[0].ctx); }
    uint32_t WalkFlags() const { return ordered_walk_ ? CPT_TRAVERSAL_ORDERED : 0u; }

    std::vector<Tile> tiles_;       // one per device of the row tiling (one: the whole frame)
    cpt_ctx* frame_ = nullptr;      // row tiling: the gathered frame on the first device
    int device_ = 0;
    std::vector<int> device_list_;  // SetDevices (empty: the single device_)
    uint64_t seed_ = 1234;
    uint max_recursion_depth_ = 8;
    bool ordered_walk_ = true;
    int width_ = 0, height_ = 0;
    PocaTexture env_ = 0;
    std::shared_ptr<MotionalCamera> camera_;
    std::vector<uint8_t> output_buffer_;   // BGRA8 handed to the callback
    bool output_pinned_ = false;           // output_buffer_ registered with cpt_host_register
    std::string err_;

    std::mutex mu_;                        // guards the queue and the context
    std::condition_variable cv_;
    std::deque<DispatchRayArgs> tasks_queue_;
    std::atomic<bool> running_{false};
    std::thread worker_;
};
