// context.h — host-side renderer state behind the C-ABI (the RayTracer of kernel.cuh:431-621).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rtx_amd.h"
#include "bvh_kernels.h"
#include "frame_kernels.h"
#include "scene_gen.h"
#include "soil_textures.h"

struct HostCamera {  // Camera::update outputs (kernel.cuh:103-121)
    float pos[3], dir[3], left[3], up[3];
    float yaw, pitch, focal, aperture;
    float res[2], invRes[2], fov[2], tanHalfFov[2];
    float adjustedLeft[3], adjustedUp[3], adjustedFront[3], apertureLeft[3], apertureUp[3];
};

// Device buffers of RayTracer::draw after the BVH (kernel.cu:259-398)
// Build outputs and scratch of one LBVH (bvh_build.hip).  With frame pipelining there are two,
// so frame f+1's build and camera rays run beside frame f's trace kernels.
// Bytes of an LBVH set's record arena (traverse.h): B*1024 BLAS nodes, B TLAS nodes and NP
// triangle records of 64 B.  BvhBufs::nodes is the arena; tlasNodes and triPos point into it.
inline size_t arena_bytes(size_t B, size_t NP) { return (B * 1024 + B + NP) * 64; }

struct BvhBufs {
    float4* triPos = nullptr;
    float4* triNrm = nullptr;
    float* aabbs = nullptr;
    float* batchScene = nullptr;
    uint32_t* morton = nullptr;
    uint32_t* reorder = nullptr;
    void* nodes = nullptr;
    float* tlasAabbs = nullptr;
    float* tlasScene = nullptr;
    uint32_t* tlasMorton = nullptr;
    uint32_t* tlasReorder = nullptr;
    void* tlasNodes = nullptr;
    uint32_t* counter = nullptr;
    float4* triDisp = nullptr;  // geometry motion vectors: the records' corner displacements (allocated on enable)
    // the mesh of the set's last build (rt_set_mesh): what every reader of the set goes by, the
    // context's counts being the current mesh's.  tlasNodes and triPos follow B (rt_build_bvh).
    uint32_t triCount = 0, triCountPadded = 0, B = 0;
    uint64_t meshSerial = 0;    // rt_context::meshSerial at that build
    // emitter sampling (rt_set_emitter_sampling): the set's emitter list, written behind
    // its build on the build's stream (emitter_kernels.h), so every reader of the set reads the list of
    // the build it traces.  Allocated on the first enable, by the triangle capacity.
    uint32_t* emTris = nullptr;
    float* emWeights = nullptr;
    float* emCdf = nullptr;
    uint32_t* emHeader = nullptr;
    float* emTriWeight = nullptr;    // scratch of the list build
    uint32_t* emBlockCount = nullptr;
    float* emScanSums = nullptr;
    bool emBuilt = false;       // the set's last build wrote a list; the path traces on it sample emitters
    uint32_t emCdfLen = 0;      // ... whose CDF has this length (emitter_cdf_len of that build's triCount)
    // signed distance queries (rt_set_signed_distance): the set's pseudo-normal table,
    // written behind its build on the build's stream (sdf.hip), so every reader of the set reads the table
    // of its build.  Allocated on the first enable, by the triangle capacity.
    float4* sdfTable = nullptr;       // [capTri][6]
    float4* sdfSlotNormal = nullptr;  // scratch of the table build, [capNP * 3]
    uint2* sdfSlotOthers = nullptr;   // ... [capNP * 3]; allocated last: the set is complete
    bool sdfBuilt = false;            // the set's last build wrote a table
    // the set's last build on the side stream (ensure_bvh_pair creates the events)
    hipEvent_t buildDone = nullptr;
    bool buildOnSide = false;   // the current users of the set wait for buildDone (wait_bvh)
    bool sideBuilt = false;     // buildDone has been recorded: a vertex update waits for it
    // pipelined frames: the end of the last path trace or ray query that read the set, which the next
    // build into it waits for
    hipEvent_t readDone = nullptr;
    bool readInFlight = false;
    bool dispValid = false;     // the set's build recorded a displacement (triDisp)
    bool dispTraced = false;    // ... and a path trace has applied it: later ones on that build do not
    // device ray queries on a context without a post stream: the end of the last query that read the set,
    // which a synchronous draw's prebuild into it waits for (a pipelined context records readDone instead)
    hipEvent_t queryDone = nullptr;
    bool queryInFlight = false;
};

// G-buffer sets in flight with frame pipelining: with four, frame f+4's camera rays wait for the
// denoise of f instead of f+3's for f's; 3 -> 4 measured 0.787 -> 0.771 ms per pipelined 1080p
// frame (tools/ab.sh, three repeats, profiles/r05_ab/gbuffer_sets/)
#ifndef RTX_GB_SETS  // A/B builds only (tools/abl_build.sh): 2..4 with RT_GBUFFER_SETS set alike
#define RTX_GB_SETS RT_GBUFFER_SETS
#endif
constexpr int kGbSets = RTX_GB_SETS;  // G-buffer / camera-output sets in flight with frame pipelining

// Material-table buffers (rt_context::matPool).  Any size >= 2 is correct, since a device set waits
// on the device for the readers of the buffer it writes; with 4, a host that sets once per frame
// writes the buffer last read three frames back, whose path trace ended long before.
constexpr int kMatPool = 4;

// What exists once per G-buffer / camera-output set (FrameResources::set).  Set 0 is allocated by
// rt_frame_init, the others on demand (alloc_frame_set); the events by the call that first needs them.
struct FrameSet {
    uint2* color = nullptr;     // the G-buffers; any of them may be the caller's (rt_bind_buffer)
    uint2* normal = nullptr;
    uint2* albedo = nullptr;
    uint16_t* depth = nullptr;
    uint32_t* motion = nullptr;
    // camera-kernel outputs (the camera rays of frame f+1 are traced while the shade / trace kernels
    // of frame f still read their set's hit records) and the counter block (PtWorkspace::counters)
    float4* hit0Rec = nullptr;
    float* hit0Err = nullptr;
    uint32_t* surface = nullptr;
    uint32_t* counters = nullptr;
    // the bounce queues with their hit records: a set's own when the shade kernel runs on the side
    // stream (shadeOnSide: frame f+1's shade appends to its queues while frame f's tracers and resume
    // kernels still read theirs) or ahead of a synchronous draw; a set without them uses set 0's
    PtQueue q3{}, q4{};
    float4* hitRec = nullptr;
    float* hitErr = nullptr;
    float4* pathL = nullptr;
    uint32_t* pending = nullptr;
    uint32_t* shade3 = nullptr;  // queue 3's shading list (PtWorkspace::shade3; [tuning] resumeSplit)
    bool inFlight = false;       // a denoise on the post stream reads the G-buffers (until postDone)
    bool camInFlight = false;    // the rest of a pipelined path trace reads the camera outputs (until restDone)
    hipEvent_t ptDone = nullptr, postDone = nullptr, camDone = nullptr, restDone = nullptr;
    hipEvent_t gatherDone = nullptr;  // the caller's G-buffer gathers (rt_set_gather_stream)
    hipEvent_t leanTraced = nullptr, leanDone = nullptr;  // fork and join of the split resume<3>'s lean pass
};

// Sky sets (rt_context::skySets): everything one sky generation (rtk_launch_sky) writes,
// the host values that belong to those tables, and the events that order the set's next writer behind
// its readers.  Launches hold their set's addresses by value, so with two sets or more update_sky never
// rewrites the current set: it generates into the next one in turn, behind these events (waited for on
// the device), and makes it current.  With one set the tables are rewritten in place behind host waits.
constexpr int kSkySetsMax = RT_SKY_SETS_MAX;
struct SkySet {
    float4* sky = nullptr;
    float* skyPdf = nullptr;
    float* skyCdf = nullptr;
    float4* sun = nullptr;
    float* sunPdf = nullptr;
    float* sunCdf = nullptr;
    float* skyTree = nullptr;   // light-CDF probe heaps (kSkyTreeNodes / kSunTreeNodes)
    float* sunTree = nullptr;
    float* lightSel = nullptr;  // [4] SampleLight's per-frame terms (k_light_select)
    float cosThetaMax = 1.0f, sunArea = 0.0f;
    hipEvent_t read = nullptr;      // behind the last path trace that read it, on the context stream
    hipEvent_t specRead = nullptr;  // behind the last kernels a synchronous draw launched ahead on it (side stream)
    bool readValid = false, specValid = false;
};

struct FrameResources {
    bool ready = false;
    // sky / sun (kernel.cu:280-307)
    float* solar = nullptr;
    float* limb = nullptr;
    float* cie = nullptr;
    SkySet skySet[kSkySetsMax];  // [rt_context::skySets]; skySet[skyCur] is what the next launch reads
    int skyCur = 0;
    SkySet& sky() { return skySet[skyCur]; }
    const SkySet& sky() const { return skySet[skyCur]; }
    uint64_t skySerial = 0;      // +1 per change of the current set (spec_matches: addresses are recycled)
    float* scanSums = nullptr;
    bool skyValid = false;
    rt_sky_params lastSky{};
    float sunDir[3] = {0, 1, 0};
    // soil textures (init.cu:524-577)
    uint2* texAlbedo = nullptr;
    uint2* texNormal = nullptr;
    uint16_t* texHeight = nullptr;  // SoilHeight (ushort chain; feeds only the reference's disabled displacement)
    // path-trace G-buffer (pathtrace.cuh:11-128): set[gbSet] is the set the last path trace wrote.
    // With a post stream (rt_set_post_stream) the path tracer cycles through kGbSets sets, so the
    // camera rays of frame f+1 and the rest of frame f are traced while frame f-1 is denoised;
    // synchronous draws alternate two (spec_on), and otherwise the set stays.
    FrameSet set[kGbSets];
    int gbSet = 0;
    FrameSet& cur() { return set[gbSet]; }
    const FrameSet& cur() const { return set[gbSet]; }
    uint32_t* rays = nullptr;
    uint4* ptStats = nullptr;
    unsigned long long* rayCounter = nullptr;
    // the non-buffer fields of every launch's workspace (cap, cus, block counts, chain); the buffers
    // are a FrameSet's (frame.cpp bind_workspace)
    PtWorkspace ws{};
    uint32_t* lastCounters = nullptr;  // the block of the last path trace (RT_ARR_PT_QUEUE)
    // serial frames: three counter blocks in turn, syncCount[0] = set[0].counters; the resolve of a
    // frame using block b zeroes block b + 2 (syncZeroed), so the camera kernel of the frame after
    // next needs no memset — and the next frame's, traced ahead (spec), has a zeroed block of its own
    uint32_t* syncCount[3] = {};
    int syncIdx = 0;
    bool syncZeroed[3] = {};
    // synchronous draws: the next frame's camera rays traced ahead, beside this frame's bounces and
    // denoise, into the other G-buffer set (frame.cpp launch_spec_camera); the next rt_path_trace
    // uses them when its launch parameters equal `p`, and traces them again otherwise
    struct Spec {
        bool valid = false;
        bool shade = false;  // the shade kernel went ahead too
        int block = 0;
        uint64_t epoch = 0;  // the geometry epoch of the LBVH they were traced on
        uint64_t matSerial = 0;  // rt_context::matSerial of the material table they read
        uint64_t skySerial = 0;  // FrameResources::skySerial of the sky set they read
        PathTraceParams p{};
    } spec;
    bool specReady = false;          // set 1's buffers and the events exist (ensure_sync_spec)
    bool gbBound = false;            // a G-buffer is the caller's (rt_bind_buffer): no set rotation, synchronous frames in set 0
    unsigned long long* specRayCounter = nullptr;  // the rays of the launches ahead (folded in when used)
    int specCounts = 0;  // specRayCounter holds: 0 nothing, 1 the counts of used launches (to fold), 2 dropped ones
    // cumulative, host only (RT_ARR_SPEC_STATS): launches ahead made, used by the next draw, and
    // discarded unused; launched == reused + dropped + (spec.valid ? 1 : 0) at any time
    uint32_t specLaunched = 0, specReused = 0, specDropped = 0;
    int lastSlot = 0;                  // slot of the last path trace (RT_ARR_PT_Q*)
    // queue 3's length after the last serial path trace, copied to pinned host memory behind it
    // (the fused chain's on/off choice for serial frames)
    unsigned long long* q3Host = nullptr;  // {length, tag} stored by k_pt_resolve (poll_q3)
    uint32_t q3Tag = 0;                    // tag of the serial frame whose length is pending
    bool q3Pending = false;
    uint32_t lastQ3 = 0;
    bool lastChain = false;  // the last path trace ran the fused k_pt_chain (rt_info.lastChain)
    HistCamera hist{};
    bool histValid = false;
    // denoise + post (denoising.cu, postprocessing.cu)
    uint2* colorB = nullptr;       // ping-pong partner of the set's color
    uint2* accum = nullptr;        // AccumulationColorBuffer (the latest)
    uint2* accumAlt = nullptr;     // the list chain writes this one and swaps (null: in place only)
    bool accumBound = false;       // accum is the caller's (rt_bind_buffer): the list chain copies back
    uint2* histBuf[2] = {};        // HistoryColorBuffer pair: histBuf[histIdx] is the latest, TemporalFilter2
    int histIdx = 0;               // writes the other one, then they swap roles
    uint16_t* histDepth = nullptr; // HistoryDepthBuffer
    uint16_t* noise8 = nullptr;
    uint16_t* noise16 = nullptr;
    uint32_t* chainCounter = nullptr;  // k_downscale_chain's finished-workgroup count (re-armed by its last one)
    uint32_t* tileList = nullptr;  // the noise-gated passes' active-tile lists (denoise.hip)
    uint32_t tileCap = 0;
    int tileParity = 0;            // counter set of the next list frame
    uint2* c4 = nullptr;
    uint2* c16 = nullptr;
    uint2* c64 = nullptr;
    uint2* bloom4 = nullptr;       // BloomBuffer4 / BloomBuffer16 (postprocessing.cu:73-88)
    uint2* bloom16 = nullptr;
    uint32_t* histogram = nullptr;
    float* exposure = nullptr;
    uint2* scaledA = nullptr;
    uint2* scaledB = nullptr;
    uint32_t* rgba = nullptr;
    uint32_t* outRgba = nullptr;   // where the last rt_denoise_post wrote RGBA8 (rgba or a draw target)
    uint32_t outPitch = 0;         // its row pitch in pixels
    uint32_t* drawTarget = nullptr;  // set by rt_draw_device for the frame it enqueues
    uint32_t drawPitch = 0;
    float4* hdr = nullptr;
    uint2* renderColor = nullptr;  // buffer that currently holds RenderColorBuffer
    uint2* scaledColor = nullptr;  // buffer that currently holds ScaledColorBuffer
    double lastDrawTime = -1.0;    // wall clock of the previous rt_draw (s)
    float drawDt = -1.0f;          // this rt_draw's frame time (ms), taken once by UpdateFrame
};

struct InputState {  // InputControl (inputControl.cu:8-25) + RayTracer::cursorReset (kernel.cuh:465)
    float moveSpeed = 0.01f;
    float cursorMoveSpeed = 0.001f;
    double xpos = 0, ypos = 0;
    bool moveW = false, moveS = false, moveA = false, moveD = false, moveC = false, moveX = false;
    float deltax = 0, deltay = 0;
    bool cursorReset = true;
};

struct rt_context {
    // ---- settings (GlobalSettings, globalSettings.h:5-22) + extensions
    int screenW = 1920, screenH = 1080;
    int renderW = 1920, renderH = 1080;
    int histW = 1920, histH = 1080;   // historyRenderWidth / Height (kernel.cu:83-84): previous frame's size
    int allocW = 1920, allocH = 1080; // render size every render-size buffer is allocated for (the max)
    int allocStripRows = 1080;        // strip rows the path-trace workspace is allocated for
    bool fullFrame = true;            // no strip split: dynamic resolution may resize the frame
    bool useDynamicResolution = true;
    float targetFps = 60.0f;
    int maxWidth = 3840, maxHeight = 2160, minWidth = 640, minHeight = 480;
    std::string inputMeshFileName, inputCameraFileName, cameraSaveFileName;
    std::vector<std::string> inputTextureFileNames;
    bool loadCameraAtInit = false;
    int chunkDim = 1;
    uint32_t maxTriangles = 0, maxVertices = 0;  // [scene] maxTriangles / maxVertices: rt_set_mesh's capacity (0: the init mesh)
    std::string meshFile;  // [scene] meshFile: meshProcessor .bin instead of the procedural scene
    int spp = 1;
    int bvhThreads = 0;  // LBVH workgroup shape: 0 = by batch count, 512 or 1024 ([render] bvhThreads)
    int stripY0 = 0, stripRows = -1;  // [render] stripY0/stripRows: screen-strip split
    int stripCount = 1, stripIndex = 0;  // [render] stripCount/stripIndex: interleaved row blocks (row_of)
    int device = -1;
    int materialOverride = -1;  // [render] materialOverride: one material for every triangle (tests)
    // [debug] fault injection (tests): a batch whose TLAS leaf box is never published, and the TLAS
    // workgroup's wait bound (rt_device.h report_status)
    uint32_t bvhSkipPublish = 0xFFFFFFFFu;
    int bvhSkipBuilds = -1;  // [debug] bvhSkipPublishBuilds: the fault applies to this many builds (-1: all)
    float bvhWaitMs = 1000.0f;
    bool sdfOn = false;      // [render] signedDistance / rt_set_signed_distance: builds write a pseudo-normal table
    int closestStack = 32;   // [debug] closestStack: stack entries of a closest-point query's lanes (2..kClosestStackMax)
    uint32_t buildSeq = 0;   // LBVH builds issued so far (a timeout report names the build)
    // [tuning] scheduling knobs (A/B aids, config only; the defaults are the measured best,
    // DESIGN.md §7): the device-buffer arena, plain prioritised streams instead of CU-masked ones,
    // the queue tracers' workgroups per CU (0: automatic), the bounce-chain choice (0 off, 1 serial
    // frames with a short queue 3, 2 always), the shade kernel on the side stream, and the
    // pipelined frame's issue points (-1: automatic)
    struct Tuning {
        bool arena = true;
        bool prioStreams = false;
        int tracePerCu = 0, trace4PerCu = 0, trace3ShortPerCu = 2;
        int chain = 1;
        bool shadeOnSide = true;
        int shadeBlocksPerCu = 0;  // k_pt_shade0's grid per CU (0: its residency)
        int overlapAfter = -1, cameraAfter = -1;
        bool syncSpec = true;   // synchronous draws trace the next frame's camera rays ahead
        int specChain = -1;     // ... and their bounces with the fused chain (1), the four kernels (0) or by queue 3's length (-1)
        int specAfter = 1;      // ... the next camera rays after kernel k of this frame (1 shade, 2 trace<3>, ..)
        int specShade = 2;      // ... and the next frame's shade kernel after them: 0 never, 1 beside the lean kernels, 2 always
        int specShadePerCu = 2; // ... that shade kernel's grid per CU (0: its residency)
        int specTracePerCu = 2; // ... this frame's bounce chain / queue-3 tracer at so many workgroups per CU (0: as usual)
        int dnSplit = 0;        // the denoise list passes at two threads per pixel: 0 never, 1 synchronous frames, 2 always
        bool dnFold = false;    // the last a-trous pass over list 1 only, its other tiles written by the first
        // resume<3> of the four-kernel bounce chain: 0 one kernel over the queue in order, 1 split into the
        // shading list's kernel and a lean pass on the same stream, 2 the lean pass on a stream of its own
        // in pipelined one-GPU frames (elsewhere as 1); the default is the fastest measured
        int resumeSplit = 2;
    } tune;

    std::string err;
    bool inited = false;
    rt_params params{};
    rt_camera camera{};
    int nextFrame = 1;     // frameNum of the next draw (kernel.cu:64 starts at 1)
    int lastFrame = 0;
    float deltaMs = 16.667f;
    InputState input;

    // ---- scene
    rtscene::SceneMesh mesh;  // the current mesh's counts (rt_set_mesh); the host arrays are rt_init's only
    uint32_t B = 0, nv = 0;
    // what every mesh-sized buffer is allocated for ([scene] maxTriangles / maxVertices)
    uint32_t capTri = 0, capNP = 0, capB = 0, capNV = 0;
    uint64_t meshSerial = 0;  // +1 per rt_set_mesh: a set's first build on a new mesh clears its arena

    // ---- device
    int cuCount = 0;                   // the device's CUs (LBVH workgroup shape)
    uint64_t wallTicksPerMs = 100000;  // s_memrealtime rate (hipDeviceAttributeWallClockRate)
    uint32_t* status = nullptr;        // pinned host words the kernels report failures into (kStatus*)
    hipStream_t stream = nullptr;      // stream every stage is enqueued on
    hipStream_t ownStream = nullptr;   // the one rt_init created (destroyed by rt_destroy)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t postStream = nullptr;  // optional: denoise + post run here (rt_set_post_stream)
    hipStream_t ownPostStream = nullptr;  // created by an asynchronous rt_draw_device (destroyed by rt_destroy)
    hipStream_t sideStream = nullptr;  // pipelining: LBVH build + camera rays of the next frame
    hipStream_t leanStream = nullptr;  // pipelining: the forked lean pass of the split resume<3> (resumeSplit 2)
    hipEvent_t overlapEv = nullptr;
    rt_collective_fn hook = nullptr;     // multi-GPU strip-local denoise exchanges (rt_set_collective_hook)
    void* hookArg = nullptr;
    uint32_t hookStages = (1u << RT_HOOK_HISTOGRAM) | (1u << RT_HOOK_ROWS);  // rt_set_hook_stages
    hipStream_t gatherStream = nullptr;  // optional: the caller's G-buffer gathers (rt_set_gather_stream)
    bool gatherOn = false;               // gatherStream is set (it may be the null stream)
    bool postGather = false;             // the pending denoise also waits for its set's gatherDone
    BvhBufs bvh[2];
    int bvhSet = 0;                      // the set the next path trace, ray query and download read
    BvhBufs& lbvh() { return bvh[bvhSet]; }
    const BvhBufs& lbvh() const { return bvh[bvhSet]; }
    bool bvhPrebuilt = false;  // synchronous draws: the next frame's LBVH is being built into set bvhSet ^ 1
    uint64_t prebuiltEpoch = 0;  // ... from the geometry of this epoch; a draw at another epoch rebuilds
    // animated geometry (rt_update_vertices*).  The build's gather and the normals
    // kernels are the only device readers of dVerts / dNormals, so there is one vertex set: an update
    // is enqueued behind the last build of every stream and the next build waits for geomDone.
    uint64_t geomEpoch = 0;             // 0 after rt_init, +1 per update
    hipEvent_t geomSrc = nullptr;       // the context stream's work up to an update without a ready event
    hipEvent_t geomDone = nullptr;      // the last update's end
    hipStream_t geomStream = nullptr;   // ... and the stream it ran on
    bool geomDoneValid = false;         // geomDone is recorded and a stream may still have to wait for it
    uint32_t* dCornerSlot = nullptr;    // corner -> slot in the vertex -> corner CSR (dAdjCorner's inverse)
    float* dContrib = nullptr;          // the corners' normal contributions in CSR order (geometry.hip)
    float* dVertStage = nullptr;        // rt_update_vertices' / rt_set_mesh's host positions, rt_time_stage(5, 6)'s copy
    // rt_set_mesh* (mesh.hip): the index staging and the adjacency sort's scratch, allocated by rt_init
    uint32_t* dIdxStage = nullptr;
    uint32_t* dSortKeys[2] = {};
    uint32_t* dSortVals[2] = {};
    uint32_t* dSortTable = nullptr;
    uint32_t* dMeshBad = nullptr;
    hipEvent_t* meshMarks = nullptr;    // set only inside rt_time_mesh_set: {start, after ingest, after adjacency, end}
    // geometry motion vectors (rt_set_geometry_motion): the motion buffer of the first
    // path trace on a build follows the vertices' displacement since the previous build.  dPrevVerts
    // is written by the first update after a build (k_geom_vertices) and read by the displacement
    // kernel behind the next build, dVerts' own readers and writers: the same orderings cover it.
    bool geomMotion = false;            // [render] geometryMotion / rt_set_geometry_motion
    float* dPrevVerts = nullptr;        // the whole mesh's positions at epoch prevVertsEpoch
    bool prevVertsValid = false;        // ... saved while the feature was on
    uint64_t prevVertsEpoch = 0;
    bool built = false;                 // an LBVH has been built, at geometry epoch builtEpoch (the last build's)
    uint64_t builtEpoch = 0;
    // skinned meshes (rt_set_skin / rt_pose_skin*): null until the first rt_set_skin, and
    // then nothing here is allocated or launched.  A pose runs k_skin_vertices (skin.hip) on the update
    // stream into dSkinned and feeds that to the whole-mesh vertex update, so dSkinned has the ordering of
    // an update's source and dVerts' (geomDone); the skin's arrays are written behind a wait for every stream.
    bool skinSet = false;               // a skin is set (rt_set_mesh* drops it)
    uint32_t skinJoints = 0;            // its joint count; its vertex count is nv
    float* dSkinRest = nullptr;         // [capNV * 3] the bind pose
    uint16_t* dSkinJoints = nullptr;    // [capNV * 4]
    float* dSkinWeights = nullptr;      // [capNV * 4]
    float* dSkinned = nullptr;          // [capNV * 3] the last pose's positions
    float* dSkinMats = nullptr;         // [RT_SKIN_JOINTS_MAX * 12] rt_pose_skin's matrices (identity after rt_set_skin)
    // per-triangle materials (rt_set_triangle_materials): null until the first set and after a reset,
    // and then every launch is the one of a context without the feature.  The pool below keeps the
    // allocation across resets; the host copy gives the census of ids (triMatCount) and from it the
    // kernel classes (rt_material_classes) without a device read
    uint8_t* dTriMat = nullptr;         // the current table (matPool[matCur].ids) or null; 3 past what was set
    std::vector<uint8_t> triMatHost;    // [triCount]
    uint32_t triMatCount[256] = {};     // triangles per id
    uint32_t triMatClasses = 0;         // RT_MAT_CLASS_* bits of the ids present (after a device set: as declared)
    // The tables (rt_set_triangle_materials_device, materials.hip).  Launches hold
    // their table's address by value, so a device set never writes the current table: it writes the
    // next buffer of this pool, in turn, behind the events of the path traces that read that buffer
    // (waited for on the device).  The host setters write the current buffer in place, after their
    // wait for every stream, and allocate that buffer only; the first device set allocates the rest.
    struct MatTable {
        uint8_t* ids = nullptr;         // [matBytes]: every byte an id, 3 where nothing was set
        uint32_t* census = nullptr;     // [256] triangles per id over [0, triCount), of the last device set into it
        hipEvent_t read = nullptr;      // behind the last path trace that read it, on the context stream
        hipEvent_t specRead = nullptr;  // behind the last shade kernel a synchronous draw launched ahead on it (side stream)
        hipEvent_t listRead = nullptr;  // behind the last emitter-list build that read it (the build's stream)
        bool readValid = false, specValid = false, listValid = false;
    } matPool[kMatPool];
    int matCur = 0;
    size_t matBytes = 0;                // capNP rounded up to 16
    bool matPoolReady = false;          // every buffer, census and event exists (the first device set)
    bool matDevice = false;             // the current table is a device set's: the host copy and census are stale
    uint64_t matSerial = 0;             // +1 per change of the table (spec_matches: addresses are recycled)
    uint32_t* dMatBad = nullptr;        // k_mat_set's count of undeclared ids, zero between sets
    hipEvent_t matSrc = nullptr;        // the context stream's work up to a set without a ready event
    hipEvent_t matDone = nullptr;       // the last device set's end
    // the material table (rt_set_materials): what an id means.  matCustom false (before the first set,
    // after rt_reset_materials): the reference's constants, no table reaches a launch.  The setters
    // write the one device buffer in place behind their wait for every stream; it belongs to the
    // context and outlives rt_set_mesh*
    bool matCustom = false;
    bool matEmits = false;              // an EMISSIVE entry of the custom table has a non-zero emission
    std::vector<rt_material> matHost;   // [256] the custom table's entries (empty until the first set)
    MatRecord* dMatTable = nullptr;     // [256], allocated by the first set
    // emitter sampling (rt_set_emitter_sampling): while on and the custom table emits
    // (emitter_active), every LBVH build is followed by its emitter list (BvhBufs::em*), and a path trace
    // on a set that has one runs the kNee kernels with the chance emitterQ
    bool emitterOn = false;             // [render] emitterSampling
    float emitterQ = 0.5f;              // [render] emitterProbability
    uint64_t prebuiltMatSerial = 0;     // matSerial at a synchronous draw's prebuild: its list is that table's
    // texture sets: fr.texAlbedo / fr.texNormal hold texSets chains each, set k
    // k * kTexTexels texels in.  matTex is the set each material id samples (rt_set_material_textures);
    // all zeros (matTexBound false) is no binding and reaches no launch.  A bound set index travels in
    // bits 16..23 of its id's MatRecord::typeFlags, so the device table is rewritten when either the
    // material table or the binding changes, and a binding without a custom table runs the
    // table-reading kernels over the defaults.
    int textureSets = 0;                // [scene] textureSets as parsed (0: absent); checked by rt_init
    uint32_t texSets = 1;               // the sets the context holds
    uint8_t matTex[256] = {};
    bool matTexBound = false;
    // rt_upload_texture_set_device writes a set in place on the context stream: it waits there for what
    // the other streams hold so far (texSide / texLean, recorded at the call) and they wait for texDone
    hipEvent_t texSide = nullptr, texLean = nullptr, texDone = nullptr;
    // sky sets and environment maps.  skySets: the sets the context holds.  The
    // environment is one context-owned table with its pdf (envTable / envPdf, written by the ingest,
    // environment.hip); while envActive, generating a sky set copies it where k_sky would run.  Every
    // write of a sky set and of the environment table runs on one stream (sky_stream()), so the table
    // needs no events of its own.
    int skySetsCfg = 0;                 // [scene] skySets as parsed (0: absent); checked by rt_init
    int skySets = 1;
    bool envActive = false;
    float4* envTable = nullptr;         // [kSkySize], allocated by the first rt_set_environment*
    float* envPdf = nullptr;
    int* envRowY = nullptr;             // the LATLONG ingest's scratch (EnvIngestParams)
    float* envRowW = nullptr;
    uint32_t* envRuns = nullptr;
    float4* envRowSums = nullptr;
    size_t envRowSumsRows = 0;          // rows envRowSums holds
    void* envStage = nullptr;           // rt_set_environment's copy of the caller's image
    size_t envStageBytes = 0;
    hipEvent_t envSrc = nullptr;        // the context stream's work up to a device set without a ready event
    hipEvent_t envDone = nullptr;       // the last device set's end
    // device ray queries (rt_trace_rays_device, trace_rays.hip): the kernel's fetch counters (kParts,
    // 64 B apart; zeroed on the context stream ahead of each launch: queries on one stream serialise,
    // and the setters that change the stream drain it)
    uint32_t* queryFetch = nullptr;
    // frame pipelining: rt_denoise_post(f) is enqueued on the post stream only once the next
    // path trace has enqueued kernel `overlapAfter` (so it fills the trace stages' idle tails), or
    // at the next host read / denoise call, whichever comes first
    bool postPending = false;
    int postPendingSet = 0;
    int overlapAfter = 1;  // after k_pt_shade0: measured best at 1-8 ranks
    int cameraAfter = 3;   // the next frame's camera rays start after this frame's kernel cameraAfter
                           // ends (0: no gate; 1 GPU), kernel 2 = trace<3> on 2 GPUs, kernel 3 =
                           // resume<3> on more (set by rt_set_post_stream)
    hipEvent_t cameraGate = nullptr;
    hipEvent_t specGate = nullptr, specDone = nullptr;  // synchronous draws' camera rays traced ahead
    bool cameraGated = false;
    // pipelined frames: the shade kernel follows the camera kernel on the side stream (set by
    // rt_set_post_stream), so the next frame's shading runs beside this frame's tracers;
    // the context stream keeps trace<3> .. resolve
    bool shadeOnSide = false;
    DenoisePostParams postParams{};
    hipEvent_t* ptMarks = nullptr;  // set only inside rt_time_path_trace_kernels
    hipEvent_t* dnMarks = nullptr;  // the denoise marks of the frame the last marked path trace traced
    // rt_frame_marks_begin: events around the marked kernels of the next markFrames frames (path trace
    // and denoise / post: 2 * kFrameKernels ring entries per frame)
    std::vector<hipEvent_t> markPool, markRing;  // ring: pool entries of the marked kernels, else null
    uint32_t markMask = 0;
    int markFrames = 0, markNext = 0;
    float* dVerts = nullptr;
    float* dNormals = nullptr;
    uint32_t* dIdx = nullptr;
    uint32_t* dAdjOff = nullptr;
    uint32_t* dAdjCorner = nullptr;
    uint8_t* dBlueNoise = nullptr;
    float4* dHits = nullptr;
    float4* dHitNrm = nullptr;
    float4* dHitFake = nullptr;
    uint32_t* dHitStats = nullptr;
    FrameResources fr{};  // path-trace / denoise / post buffers (frame_kernels.h)

    std::vector<void*> allocations;
    std::vector<hipEvent_t> events;  // every event the context created (rt_event), destroyed by rt_destroy
    // device arena (rt_dalloc_bytes): buffers up to kArenaMaxBuffer are carved from 256-MiB chunks
    char* arenaPtr = nullptr;
    size_t arenaUsed = 0, arenaCap = 0;
};

// helpers shared by the C-ABI translation units
#define HIP_TRY(ctx, expr)                                                            \
    do {                                                                              \
        hipError_t e__ = (expr);                                                      \
        if (e__ != hipSuccess) {                                                      \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);          \
            return RT_ERR_HIP;                                                        \
        }                                                                             \
    } while (0)

#define RT_TRY(expr)                         \
    do {                                     \
        if (int rc__ = (expr)) return rc__;  \
    } while (0)

int rt_dalloc_bytes(rt_context* ctx, void** p, size_t bytes);  // hipMalloc, freed by rt_destroy
template <typename T>
int dalloc(rt_context* ctx, T** p, size_t bytes) {
    void* q = nullptr;
    const int rc = rt_dalloc_bytes(ctx, &q, bytes);
    *p = (T*)q;
    return rc;
}
template <typename T>
int dalloc_once(rt_context* ctx, T*& p, size_t bytes) {  // a buffer allocated on first use, kept from then on
    return p ? RT_OK : dalloc(ctx, &p, bytes);
}
int rt_event(rt_context* ctx, hipEvent_t& e, bool timing = false);  // context.cpp: created if null, destroyed by rt_destroy
int rt_create_stream(rt_context* ctx, hipStream_t* s, bool high);  // context.cpp: renderer streams
extern "C" int ensure_bvh_pair(rt_context* ctx);  // frame.cpp: second LBVH set, side stream, build events
int rt_frame_init(rt_context* ctx);  // frame.cpp: sky tables, textures, G-buffers
int rt_time_sky_generation(rt_context* ctx);  // frame.cpp: rt_time_stage(7)'s launch, one generation into a spare sky set
int rt_regenerate_sky(rt_context* ctx);  // frame.cpp: the sky tables again from the current parameters and environment
// the stream every sky-set and environment-table write runs on: the side stream of a pipelined context,
// where the builds and camera kernels run, and the context stream otherwise (DESIGN.md §3.1's choice)
inline hipStream_t sky_stream(const rt_context* ctx) { return ctx->postStream ? ctx->sideStream : ctx->stream; }
int sync_streams(rt_context* ctx, bool report = true);  // frame.cpp: context, post and side streams (report: RT_ERR_DEVICE)
void poll_q3(rt_context* ctx);       // frame.cpp: the last serial frame's queue-3 length, if stored
int check_device_status(rt_context* ctx);  // frame.cpp: kernel failure reports (RT_ERR_DEVICE)
bool strip_local_denoise(const rt_context* ctx, uint32_t& a, uint32_t& b);  // frame.cpp: next denoise's rows
extern "C" int copy_rgba_out(rt_context* ctx, void* dst);  // frame.cpp: the last frame's RGBA8 to host memory
extern "C" size_t rt_alloc_bytes(const rt_context* ctx, int name);  // frame.cpp: allocated size of a render buffer
int alloc_bvh_set(rt_context* ctx, BvhBufs& b);  // context.cpp: an LBVH set's buffers, arena cleared and placed
int build_bvh(rt_context* ctx, int set, hipStream_t stream);  // context.cpp: the LBVH of the current geometry into bvh[set]
bool closest_distance_ok(float max_distance);  // closest.cpp
extern "C" int wait_bvh(rt_context* ctx);  // context.cpp: context stream waits for the LBVH build
extern "C" int ensure_emitter_lists(rt_context* ctx);  // context.cpp: the existing LBVH sets' emitter-list buffers
extern "C" int ensure_sdf_tables(rt_context* ctx);  // context.cpp: the existing LBVH sets' pseudo-normal tables
inline bool emitter_active(const rt_context* ctx) { return ctx->emitterOn && ctx->matCustom && ctx->matEmits; }
extern "C" int ensure_geometry_motion(rt_context* ctx);  // context.cpp: dPrevVerts and the existing LBVH sets' triDisp
const char* skin_shape_fault(const rt_skin* s);  // skin.cpp: what is wrong with a skin's pointers or counts, or null
const char* skin_content_fault(const rt_skin* s, uint32_t& vertex);  // ... or with its joints and weights, and at which vertex
std::string rt_data_dir();
void rt_camera_update(const rt_camera& in, int renderW, int renderH, HostCamera& c);
void rt_input_control_update(rt_context* ctx, float deltaTime);  // input.cpp
TraceCamera rt_trace_camera(const HostCamera& c);
