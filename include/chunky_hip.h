/* chunky_hip.h — C ABI of the MI355X-native Chunky path-tracing hot path.
 *
 * This is the boundary a Chunky plugin binds instead of JOCL/OpenCL: plain pointers and sizes,
 * no C++ or torch types.  Each entry point names the reference interface it replaces
 * (paths relative to /root/reference/src/main/java/dev/thatredox/chunkynative/, "J/", and
 * /root/reference/src/main/opencl/kernel/include/, "K/").  INTEGRATION.md shows the JNI stub a
 * maintainer adds on the Java side.
 *
 * Conventions:
 *   - every function returns 0 on success, a negative chunky_status on failure; the message is
 *     available from chunky_last_error() on the calling thread.  Nothing aborts the process.
 *   - host arrays are COPIED before the call returns (the reference creates every buffer with
 *     CL_MEM_COPY_HOST_PTR / blocking writes: J/opencl/util/ClIntBuffer.java:23-25); the caller
 *     keeps ownership.  Zero-length int arrays are legal (ClIntBuffer.java:15-18).
 *   - handles may be destroyed from any thread, at most once (the reference frees from a GC
 *     cleaner thread: J/util/NativeCleaner.java:45-53).  Calls on one context are serialised by
 *     an internal mutex (the reference's renderLock, J/opencl/OpenClPathTracingRenderer.java:56).
 *   - there is no CPU fallback: without a HIP device chunky_init fails with CHUNKY_E_NO_DEVICE.
 */
#ifndef CHUNKY_HIP_H
#define CHUNKY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum chunky_status {
    CHUNKY_OK = 0,
    CHUNKY_E_INVALID = -1,    /* bad argument / handle */
    CHUNKY_E_NO_DEVICE = -2,  /* no HIP device, or device index out of range */
    CHUNKY_E_HIP = -3,        /* a HIP runtime call failed (message has the HIP error string) */
    CHUNKY_E_STATE = -4,      /* call sequence error (e.g. render before a scene is complete) */
    CHUNKY_E_ABORTED = -5     /* the postRender callback asked to stop */
} chunky_status;

typedef struct chunky_ctx chunky_ctx;        /* one GPU: J/opencl/renderer/RendererInstance.java */
typedef struct chunky_scene chunky_scene;    /* device copies of the packed scene: J/opencl/renderer/ClSceneLoader.java */
typedef struct chunky_render chunky_render;  /* one render target + camera: OpenClPathTracingRenderer.render locals */

/* ---- device (replaces RendererInstance.java:31-110: platform/device enumeration, context, queue) */
int chunky_device_count(void);
int chunky_device_name(int device, char* buf, int buf_len);
int chunky_init(int device, chunky_ctx** out);
int chunky_shutdown(chunky_ctx* ctx);
/* Several GPUs behind ONE context, in one process (SURVEY.md section 8b "init(device_ids[], n)", 8e; the reference holds one
 * cl_context per JVM, RendererInstance.java:74-101, and a Chunky JVM is one process).  The handle is an ordinary chunky_ctx:
 * every scene / render / filter entry point accepts it.  A scene created on it is replicated on every member (each chunky_scene_set_*
 * uploads to all of them); a render target created on it is cut into blocks of 16 x 16 pixels dealt round-robin to the members
 * (member i renders blocks b with b % n == i, `gid` stays the global pixel index, so seeds and results are those of one GPU);
 * chunky_render_passes enqueues every member's share and returns; chunky_render_read is the one exchange per read-back: each
 * member packs the blocks it owns and sends them to member 0 (one grouped RCCL send / receive over xGMI, or peer copies where
 * RCCL is not available: chunky_group_transport; 1/n of the image per member) where they are scattered into the image, which is
 * then read back — bit for bit the one-GPU image.  `devices` may name a device more than once (members then share it: how the path is tested on a 1-GPU box).
 * chunky_shutdown destroys the members. */
int chunky_group_create(const int* devices, int n, chunky_ctx** out);
/* Members of a context: 1 for chunky_init's, n for chunky_group_create's. */
int chunky_group_size(chunky_ctx* ctx);
/* Device index of member i. */
int chunky_group_device(chunky_ctx* ctx, int i);
/* How each member's share of a read-back reaches member 0, decided once in chunky_group_create (no reference counterpart; the
 * reference is single-device): out[i] = CHUNKY_PEER_LOCAL (member 0 itself, or a member on member 0's device), CHUNKY_PEER_DIRECT
 * (hipDeviceEnablePeerAccess succeeded: hipMemcpyPeerAsync writes member 0's memory over xGMI), CHUNKY_PEER_STAGED (the devices
 * report no peer access: the runtime stages the copy through the host), or -(hipError_t) when enabling it failed (the copy still
 * works, staged).  n = room in out, at least chunky_group_size(ctx). */
#define CHUNKY_PEER_LOCAL 0
#define CHUNKY_PEER_DIRECT 1
#define CHUNKY_PEER_STAGED 2
int chunky_group_peer_status(chunky_ctx* ctx, int* out, int n);
/* What carries the one exchange per read-back of a group (no reference counterpart: one device, one queue,
 * RendererInstance.java:74-101; SURVEY.md section 8e "a single RCCL reduce of per-tile radiance over xGMI").
 * chunky_group_create binds RCCL at run time (dlopen: the collective library is not a link dependency; CHUNKY_RCCL_LIB names
 * the file, else librccl.so.1) and opens one communicator over the members (ncclCommInitAll) when they are distinct devices:
 *   CHUNKY_TRANSPORT_RCCL_SENDRECV  each member packs the blocks it owns and ncclSend's them, member 0 posts the matching
 *                                   ncclRecv's — ONE grouped RCCL operation per read-back, 1/n of the image per member —
 *                                   and scatters them into the image (the default when the communicator exists);
 *   CHUNKY_TRANSPORT_RCCL_REDUCE    ONE ncclReduce(sum) of the members' zero-padded framebuffers onto member 0, as SURVEY
 *                                   words it: every member moves the whole image, x + 0 = x keeps it bit-identical;
 *   CHUNKY_TRANSPORT_PEER_COPY      the packed blocks travel by hipMemcpyPeerAsync (chunky_group_peer_status says how):
 *                                   the fallback when RCCL cannot be bound, the communicator cannot be created (members
 *                                   sharing a device), or an RCCL call fails later — the render survives and `detail` says why.
 * All three leave the same bytes in the pixels the group's members own (with an outer chunky_render_set_shard split the REDUCE
 * form also zeroes the pixels of member 0's image that no member owns; the other two leave them alone).
 * First contact is checked, not assumed: before RCCL becomes a group's transport, chunky_group_create sends a known pattern from
 * every member to member 0 through the new communicators and compares the bytes; an error, a wrong byte or an exchange that does
 * not finish makes the group start on peer copies, with the reason in `detail`.  No exchange waits in the driver behind an RCCL
 * kernel: the library polls the members' streams and the communicators' asynchronous errors, and after 30 s without completion
 * (or on any RCCL error) it calls ncclCommAbort FIRST — the one call that ends a collective whose peer or link died — then drains
 * the streams and repeats that read-back, and every later one, on peer copies.
 * chunky_group_transport reports the transport the next read-back will use and a human-readable detail (library file and
 * version, or the reason for the fallback); chunky_group_set_transport picks one (CHUNKY_E_STATE when it needs a communicator
 * that does not exist).  On a chunky_init context: PEER_COPY, nothing to exchange.
 * Environment: the shipping library reads ONE variable, CHUNKY_RCCL_LIB (a deployment's own librccl file).  Everything else —
 * the initial transport, the one-GPU rigs of tests/test_gpu_rccl_transport.py (CHUNKY_GROUP_TRANSPORT, CHUNKY_GROUP_SELF_EXCHANGE,
 * CHUNKY_GROUP_NO_PROBE, CHUNKY_GROUP_TIMEOUT_MS, CHUNKY_RCCL_TRY_SHARED) and the tuning overrides of the octree / BVH re-layouts —
 * exists only in a build with -DCHUNKY_TUNING (chunkyclplugin_amd/native.py build_tuning), never in what a JVM loads. */
#define CHUNKY_TRANSPORT_PEER_COPY 0
#define CHUNKY_TRANSPORT_RCCL_SENDRECV 1
#define CHUNKY_TRANSPORT_RCCL_REDUCE 2
int chunky_group_transport(chunky_ctx* ctx, int* transport, char* detail, int detail_len);
int chunky_group_set_transport(chunky_ctx* ctx, int transport);
const char* chunky_last_error(void);
/* Library identity: "chunky-hip <version> gfx950". */
const char* chunky_version(void);

/* ---- scene upload (replaces the clCreateBuffer/clCreateImage sites of ClSceneLoader.java:52-150,
 *      ClIntBuffer.java:14-26, ClTextureLoader.java:50-67, ClSky.java:28-61) */
int chunky_scene_create(chunky_ctx* ctx, chunky_scene** out);
int chunky_scene_destroy(chunky_scene* scene);

/* References inside the scene data (the reference kernel follows them unchecked: clCreateBuffer copies ints, nothing validates them):
 *   - octree branch values and BVH node links are checked on upload (CHUNKY_E_INVALID: outside the array, cyclic, deeper than 64);
 *   - an octree leaf whose block pointer lies beyond the block palette renders as air;
 *   - a block whose model pointer, primitive count or material pointers leave their palettes never intersects, like a block of
 *     unknown model type (K/block.h:44-47);
 *   - an entity BVH whose leaves leave the triangle palette, or whose triangles' materials leave the material palette, makes
 *     chunky_render_passes / _run / _preview fail with CHUNKY_E_INVALID.
 * Well-formed data is unaffected.  The palettes may arrive in any order; the checks run when a render call first sees them together.
 * Any setter below (chunky_scene_load_octree and chunky_scene_write_atlas_tile included) may be called again at any time, also on a
 * scene that render targets have rendered from: launches already queued finish on the old contents, the next launch sees the new ones. */
/* octreeData after the leaf remap of ClSceneLoader.java:52-63 + octreeDepth (getOctreeData/getOctreeDepth) */
int chunky_scene_set_octree(chunky_scene* scene, const int32_t* tree, int64_t n_ints, int depth);
/* Same, from Chunky's raw PackedOctree.treeData + blockMapping: performs the remap
 * `i>0 || -i>=len ? i : -blockMapping[-i]` of ClSceneLoader.java:56-58 on the way in (a22). */
int chunky_scene_load_octree(chunky_scene* scene, const int32_t* tree_data, int64_t n_ints, int depth,
                             const int32_t* block_mapping, int64_t n_mapping);

typedef enum chunky_palette {
    CHUNKY_PALETTE_BLOCK = 0,    /* getBlockPalette():    2 ints/block      (PackedBlock.java:80-85) */
    CHUNKY_PALETTE_MATERIAL = 1, /* getMaterialPalette(): 6 ints/material   (PackedMaterial.java:89-100) */
    CHUNKY_PALETTE_AABB = 2,     /* getAabbPalette():     1+13n ints/model  (PackedAabbModel.java:41-47) */
    CHUNKY_PALETTE_QUAD = 3,     /* getQuadPalette():     1+15n ints/model  (PackedQuadModel.java:39-45) */
    CHUNKY_PALETTE_TRIG = 4      /* getTrigPalette():     1+20n ints/leaf   (PackedTriangleModel.java:28-34) */
} chunky_palette;
int chunky_scene_set_palette(chunky_scene* scene, int kind, const int32_t* data, int64_t n_ints);

typedef enum chunky_bvh { CHUNKY_BVH_WORLD = 0, CHUNKY_BVH_ACTOR = 1 } chunky_bvh;
/* getWorldBvh()/getActorBvh(): 7 ints/node (PackedBvhNode.java:16-31); {0, NaN x 6} = empty */
int chunky_scene_set_bvh(chunky_scene* scene, int which, const int32_t* nodes, int64_t n_ints);

/* Texture atlas (getTexturePalette().getAtlas()): RGBA8, [layer][y][x][4].  gfx950 has no image
 * instructions, so the atlas is a flat buffer; width/height need only cover the occupied tiles
 * (the reference allocates 8192x8192 per layer, ClTextureLoader.java:50-58; locations are
 * identical).  set_atlas allocates (and zero-fills when rgba == NULL); write_atlas_tile mirrors the
 * per-texture clEnqueueWriteImage of ClTextureLoader.java:61-66. */
int chunky_scene_set_atlas(chunky_scene* scene, const uint8_t* rgba, int width, int height, int layers);
int chunky_scene_write_atlas_tile(chunky_scene* scene, int x, int y, int layer, int w, int h, const uint8_t* rgba);
/* getSky(): skyTexture RGBA8 [h][w][4] + skyIntensity (ClSky.java:28-30,43-61) */
int chunky_scene_set_sky(chunky_scene* scene, const uint8_t* rgba, int width, int height, float intensity);
/* The emitter list CHUNKY_OPT_EMITTER_NEE samples (no reference counterpart): every octree leaf whose block is a full cube
 * with a non-zero emittance byte and no emittance texture (material flag 2), in pre-order, 4 ints each {x, y, z, level << 25 | block pointer}.  *count receives the
 * number of emitters; at most `cap` are written. */
int chunky_scene_emitters(chunky_scene* scene, int32_t* out4, int32_t cap, int32_t* count);
/* getSun(): flags, textureSize, textureLocation, intensity, altitude, azimuth (PackedSun.java:32-41) */
int chunky_scene_set_sun(chunky_scene* scene, const int32_t sun[6]);
/* Biome tints by block position (no reference counterpart: the reference multiplies tint types 1, 2 and 3 — foliage, grass, water — by
 * three fixed colours, K/material.h:61-72).  rgb3 holds size_x * size_z * 3 ints: the cell (x, z) of the octree's cell grid, x0 <= x <
 * x0 + size_x, z0 <= z < z0 + size_z, has its foliage, grass and water colour at rgb3[((z - z0) * size_x + (x - x0)) * 3 + 0 / 1 / 2].
 * Only the low 24 bits of a word are read: RGB as in a tint word.  The array is copied before the call returns.
 * Rule (CHUNKY_OPT_BIOME_TINT at 1, its default): a material of tint type t in {1, 2, 3} evaluated for a block of the octree multiplies
 * by colorFromArgb(0xFF000000 | rgb3[cell][t - 1]), where the cell is the integer cell (x, z) BlockPalette_intersectBlock receives (for a
 * leaf larger than one cell: the march point's cell); outside the rectangle it multiplies by the reference's constant.  Entity triangles
 * keep the constants, tint types 0 and 0xFF and everything else are unchanged, and record.material (the block-id image, the mattes,
 * chunky_render_trace_records) reports the block pointer the octree holds.  The image is, bit for bit, the reference's image of a
 * world in which every tinted block was replaced, cell by cell, by a copy whose material carries the constant tint 0xFF000000 | rgb.
 * rgb3 == NULL with both sizes 0 removes the map.  CHUNKY_E_INVALID: a negative size, exactly one size 0, rgb3 == NULL with a size
 * that is not 0, a non-NULL rgb3 with both sizes 0, or size_x * size_z above CHUNKY_BIOME_MAX_CELLS.  On a group the map reaches every member.
 * As every setter it may be called again at any time: launches already queued finish on the old map.
 * Served with a map: chunky_render_passes / _run (the pool kernel for pinhole and pre-generated cameras, render_lanes for the fallback
 * kernels' scenes and options), chunky_render_preview, chunky_render_trace_records, chunky_render_aov_passes and _aov_passes_ex.  The
 * matte and occlusion passes hold no colour and run as they are.  CHUNKY_E_STATE, before anything is allocated or launched, with
 * the reason in the message: phase statistics (CHUNKY_OPT_KERNEL bit 2), the extended light-transport options, a projected camera
 * on the pool kernel (CHUNKY_OPT_KERNEL bit 1 serves it), chunky_render_light_passes, chunky_render_adaptive*, chunky_selftest_render_list. */
#define CHUNKY_BIOME_MAX_CELLS (1 << 26)
int chunky_scene_set_biome_tints(chunky_scene* scene, const int32_t* rgb3, int x0, int z0, int size_x, int size_z);

/* ---- render target (replaces the buffers and the launch of OpenClPathTracingRenderer.java:67-141) */
int chunky_render_create(chunky_ctx* ctx, chunky_scene* scene, int width, int height, chunky_render** out);
int chunky_render_destroy(chunky_render* r);
/* ClCamera (ClCamera.java:33-70): projector_type 0 = pinhole with 15 floats; -1 = pre-generated rays,
 * width*height*6 floats (ClCamera.java:72-105); 1-5, 7 and 8 = a projected camera (below); any other value (6 is unassigned) is
 * rejected.
 * Types 0 and -1 are the reference's own; -1 stays the route that reproduces any of Chunky's projectors exactly. */
int chunky_render_set_camera(chunky_render* r, int projector_type, const float* settings, int64_t n_floats);

/* Projected cameras: the kernels compute the primary ray of every sample from the pass seed, with fresh jitter on every pass; no
 * table is built or uploaded.  15 floats laid out as the pinhole camera's: pos[3], m[9] (rows, ClCamera.java:42-52), then
 * settings[12] = aperture, which must be 0 (the depth of field of a projected camera is set by chunky_render_set_lens, below),
 * settings[13] and settings[14]:
 *
 *   type                         settings[13]                          settings[14]
 *   CHUNKY_PROJ_PARALLEL         origin back-off b (world units)       view scale w (world units per unit of y)
 *   CHUNKY_PROJ_FISHEYE          0                                     fov in degrees
 *   CHUNKY_PROJ_PANORAMIC        0                                     fov in degrees
 *   CHUNKY_PROJ_PANORAMIC_SLOT   fovTan (as the host computes it for pinhole)   fov in degrees
 *   CHUNKY_PROJ_STEREOGRAPHIC    0                                     scale k
 *   CHUNKY_PROJ_ODS              eye offset e (world units), signed:   vertical fov in degrees (180: the full sphere)
 *                                e > 0 the right eye, e < 0 the left
 *   CHUNKY_PROJ_ODS_STACKED      eye offset e >= 0                     vertical fov in degrees
 *
 * ODS is omnidirectional stereo: the image's width spans the full turn whatever its aspect, and each column looks from its own
 * point of the circle of radius |e| about the camera.  ODS_STACKED holds both eyes: rows py < height / 2 are the eye -e (left, on
 * top), the rest the eye +e; it needs an even height.
 *
 * A non-finite value, settings[14] <= 0, a non-zero aperture, a non-zero settings[13] where it must be 0, a negative offset or an
 * odd image height for ODS_STACKED, or n_floats != 15 is CHUNKY_E_INVALID, and the camera is left as it was.
 *
 * Per sample (pixel gid = y * width + x, the same gid on shards and group members; pass seed s):
 *   j  = ((uint)s ^ 0x9E3779B9u) + (uint)gid             the jitter's own stream: the path's state stays seed + gid advanced once,
 *   ox = rand(j); oy = rand(j)                           as on the pre-generated path (rand: K/randomness.h, in this order)
 *   x  = -width / (2 height) + (x + ox) / height,  y = -0.5 + (y + oy) / height   (the pinhole camera's roundings)
 * then, in float with rad(v) = v * 0.0174532924f:
 *   PARALLEL        o = (w x, w y, -b), d = (0, 0, 1)
 *   FISHEYE         ax = rad(x fov), ay = rad(y fov), a = sqrt(ax^2 + ay^2); d = a == 0 ? (0, 0, 1) : (sin a ax/a, sin a ay/a, cos a)
 *   PANORAMIC       ax = rad(x fov), ay = rad(y fov); d = (cos ay sin ax, sin ay, cos ay cos ax)
 *   PANORAMIC_SLOT  ax = rad(x fov); d = (sin ax, fovTan y, cos ax)
 *   STEREOGRAPHIC   X = k x, Y = k y, r2 = X^2 + Y^2; d = (2X, 2Y, 1 - r2) / (1 + r2)
 *   ODS             th = x * (PI_F / (width / (2 height)))   (one float division); y2 = y, eye = e
 *   ODS_STACKED     th as ODS; py < height / 2: y2 = 2 y + 0.5, eye = -e; else y2 = 2 y - 0.5, eye = e
 *                   both: ph = rad(y2 fov); d = (cos ph sin th, sin ph, cos ph cos th); o = (eye cos th, 0, -(eye sin th))
 * (o = 0 where not given), d normalised; then the lens, if one is set (below); then o and d are rotated by m and o moved by pos
 * as the pinhole camera's ray.  The exact arithmetic is
 * chunkyclplugin_amd/csrc/camera_proj.h.  Chunky's own projector classes were not at hand: these formulas follow them as this
 * project understands them, and they are this project's specification, not Chunky's.
 *
 * Equivalence: a pass with projected camera k and seed s is, bit for bit, the pass with seed s on projector type -1 fed the table
 * chunky_camera_rays(k, ..., s) returns.  chunky_render_preview uses the rays of seed 0. */
#define CHUNKY_PROJ_PARALLEL 1
#define CHUNKY_PROJ_FISHEYE 2
#define CHUNKY_PROJ_PANORAMIC 3
#define CHUNKY_PROJ_PANORAMIC_SLOT 4
#define CHUNKY_PROJ_STEREOGRAPHIC 5
#define CHUNKY_PROJ_ODS 7
#define CHUNKY_PROJ_ODS_STACKED 8
/* The width*height*6-float table (origin, direction per pixel, the layout of projector type -1) of projected camera
 * `projector_type` for the pass of seed `seed`, computed on the host with the kernels' arithmetic; needs no device.  Types 0 and
 * -1, and settings set_camera would reject, are CHUNKY_E_INVALID. */
int chunky_camera_rays(int projector_type, const float* settings, int64_t n_floats, int width, int height, int32_t seed, float* out);

/* The lens (depth of field) of the projected cameras.  chunky_render_set_lens(r, aperture, focus) gives the camera set last a
 * lens disc of radius `aperture` (world units) in focus at distance `focus`; aperture == 0 switches the lens off.  A successful
 * chunky_render_set_camera clears the lens, so the lens is set after the camera, every time.
 *   CHUNKY_E_STATE    before a camera is set, and while the camera is projector type 0 or -1 (which have their own aperture or table)
 *   CHUNKY_E_INVALID  a non-finite value, aperture < 0, or aperture > 0 with focus <= 0; the lens is left as it was
 * Like set_camera it reaches every member of a group, and it ends an adaptive run that could have been resumed.
 *
 * Per sample, with lo / ld the local origin and the normalised local direction of the projection above, just before the rotation
 * by m (float, no fused multiply-add, in this order):
 *   aperture == 0:  nothing is drawn and nothing changes
 *   otherwise:
 *     u1 = rand(j); u2 = rand(j)                  draws 3 and 4 of the jitter stream j (the path's own state stays untouched)
 *     r = sqrt(u1) * aperture
 *     theta = (float)((double)(u2 * PI_F) * 2.0)  (the pinhole lens's rounding, K/camera.h:24-27)
 *     rx = cos(theta) * r;  ry = sin(theta) * r
 *     PARALLEL (a planar lens in the origins' plane local z = -b, in focus on the plane `focus` in front of it; with b = 0 these are
 *     local z = 0 and local z = focus):
 *         off = (rx, ry, 0);  t = (0, 0, focus) - off
 *     every other type (in focus on the sphere of radius focus about lo):
 *         U = |ld.x| > |ld.y| ? (-ld.z, 0, ld.x) : (0, ld.z, -ld.y);  U = U / |U|;  V = cross(ld, U)
 *         off = U rx + V ry;  t = ld focus - off
 *     lo = lo + off;  ld = t / |t|
 * The equivalence above holds with a lens: the pass is the pass on projector type -1 fed chunky_camera_rays_lens(k, ..., s,
 * aperture, focus), the host twin of the kernels' arithmetic, which needs no device.  With aperture == 0 it returns
 * chunky_camera_rays' bytes; it refuses what chunky_camera_rays and chunky_render_set_lens refuse.  As the projections, this lens
 * is this project's specification, not a transcription of Chunky's ApertureProjector. */
int chunky_render_set_lens(chunky_render* r, float aperture, float focus);
int chunky_camera_rays_lens(int projector_type, const float* settings, int64_t n_floats, int width, int height, int32_t seed,
                            float aperture, float focus, float* out);

/* Canvas windows: a render target of width x height pixels may be declared the window at (x0, y0) of a canvas
 * of canvas_width x canvas_height.  Window pixel (x, y), local index g = y * width + x, is canvas pixel (X, Y) = (x0 + x, y0 + y),
 * canvas index G = Y * canvas_width + X.
 *
 * THE RULE.  The window target stores, at g, exactly what a canvas_width x canvas_height target with the same scene, camera, lens,
 * options and seeds stores at G — in every image any call produces, bit for bit.  Per sample: the RNG state is seed + (unsigned)G,
 * advanced once; the pinhole camera and the preview use half_width = (float)(canvas_width / (2.0 * canvas_height)), inv_height =
 * (float)(1.0 / canvas_height) and (float)X, (float)Y (the offset is added to the integer, before the conversion); the projected
 * cameras and their lens draw from ((uint)seed ^ 0x9E3779B9u) + (uint)G and read X, Y and the canvas's size (ODS_STACKED changes
 * eye at canvas_height / 2 and needs an even canvas height); the preview's crosshair is the canvas's.  A table of pre-generated rays
 * (type -1) stays window-sized, width * height * 6 floats read at g — the caller crops its table — while the RNG state still uses G.
 * Everything else stays the target's own: buffer sizes and read-back counts, the 16 x 16 block map and chunky_render_set_shard, a
 * group's split among its members, chunky_render_set_device_buffer, the gids of chunky_render_trace_records (local), matte planes.
 * No call answers CHUNKY_E_STATE because a window is set.
 *
 * Two calls look at neighbouring pixels and so cannot equal a crop near the window's edge; they run as they are:
 *   chunky_render_denoise / chunky_denoise_frame  the filter reaches as far as its A-Trous levels (2^iterations pixels): render the
 *                                                 window with an apron that wide and crop after filtering
 *   chunky_render_adaptive*                       the 3 x 3 activity neighbourhood is clipped to the window, so a pixel may stop at
 *                                                 another pass count than on the canvas; every pixel's result is still
 *                                                 chunky_render_passes(seeds[0 .. n_p)) of its canvas pixel
 *
 * chunky_render_set_canvas may be called before or after chunky_render_set_camera, and again at any time; canvas == target with
 * offsets 0 is the default and switches the window off.  Launches already queued keep the window they were enqueued with (the
 * camera travels by value).  It touches no image: a host that moves the window calls chunky_render_reset (and the other passes'
 * reset functions) itself.  Like set_camera it reaches every member of a group and ends an adaptive run that could have been resumed.
 *   CHUNKY_E_INVALID, nothing changed: a negative offset; a window that does not lie inside the canvas; canvas_width *
 *   canvas_height > INT32_MAX (G is an int); an odd canvas_height while the camera is CHUNKY_PROJ_ODS_STACKED (set_camera checks the
 *   same on the canvas's height, not the target's)
 * chunky_render_canvas reports canvas_width, canvas_height, x0, y0.  chunky_canvas_check is set_canvas' test without a target or a
 * device (projector_type: the camera's, 0 if none); chunky_selftest_canvas_pixel (a self test, like the other chunky_selftest_* entries) gives {G, X, Y} of local index g by the kernels' own helper.
 * chunky_camera_rays_window is the host twin of a projected camera on a window: the width * height * 6 table of the WINDOW's pixels;
 * with canvas == window and aperture 0 it returns chunky_camera_rays' bytes, with a lens chunky_camera_rays_lens'.
 * The Java binding does not reach these calls. */
int chunky_render_set_canvas(chunky_render* r, int canvas_width, int canvas_height, int x0, int y0);
int chunky_render_canvas(chunky_render* r, int32_t out4[4]);
int chunky_canvas_check(int width, int height, int canvas_width, int canvas_height, int x0, int y0, int projector_type);
int chunky_selftest_canvas_pixel(int width, int height, int canvas_width, int canvas_height, int x0, int y0, int32_t g, int32_t out3[3]);
int chunky_camera_rays_window(int projector_type, const float* settings, int64_t n_floats, int width, int height,
                              int canvas_width, int canvas_height, int x0, int y0, int32_t seed,
                              float aperture, float focus, float* out);

/* Ground fog (no reference counterpart; arithmetic: csrc/fog_spec.h; specification: tests/fog_port.c).
 *
 * A render target may carry one homogeneous, isotropically scattering fog layer: density sigma per block of path length inside the slab
 * y_min <= y < y_max (octree coordinates), single-scattering colour `color`.  It is path traced — multiple scattering, lit by sun and
 * sky, dimming the sun on what lies under it — by chunky_render_passes, on kernels of their own (the extended integrator with a
 * medium vertex); with fog off (the default, density 0) every call runs the kernels it ran before and writes the same bits.
 *
 * The model.  At the end of every trace of a path's own ray, hit or miss, the part of the ray inside the slab is found (up to the hit,
 * or to infinity).  If there is one, one random number u gives a free-flight distance s = -ln(1 - u) / sigma; if s is shorter than the
 * part, the path has a MEDIUM VERTEX there: throughput *= color, the sun is sampled (where sun sampling is on) with weight 1/4 x the
 * slab's transmittance towards the sun, and the path goes on in a direction uniform on the sphere; its depth counts as a bounce.
 * Otherwise the surface, or the sky, is seen at full weight.  At a surface vertex the sun ray's weight is multiplied by the slab's
 * transmittance towards the sun (to infinity), an emitter sample's by the transmittance up to the emitter.
 *
 * chunky_render_set_fog: `fog` NULL, or density 0, turns fog off; else every member is checked and the layer replaces the target's.
 * fog->size is the caller's sizeof(chunky_fog): a smaller struct than this header's that still holds `color` is taken (members added
 * later default to 0), a larger one is taken when its extra bytes are all 0.  It touches no image and reaches every member of a group;
 * like a change of options it ends an adaptive run that could have been resumed.  CHUNKY_E_INVALID, nothing changed: a non-finite
 * member, density < 0, y_min >= y_max, a colour component outside [0, 1], a size that fits neither rule.
 * chunky_render_fog reports the layer (density 0: off); out->size is set to this header's sizeof.  chunky_fog_check is set_fog's test
 * without a target or a device.
 *
 * While fog is on:
 *   chunky_render_passes            runs the fog kernels, or answers CHUNKY_E_STATE with the reason, before anything is launched or
 *                                   written, and never renders without fog: a projected camera (types 1-8; pre-generated rays, type -1,
 *                                   serve every projection), CHUNKY_OPT_KERNEL bits 0-3, CHUNKY_OPT_MAX_DEPTH above 254, a scene whose
 *                                   octree has no wide re-layout (deeper than 15 levels) or whose entity BVHs could not be re-laid
 *                                   out, a scene with a biome map while CHUNKY_OPT_BIOME_TINT is 1.  The light-transport options
 *                                   (CHUNKY_OPT_SUN_SAMPLING .. _EMITTER_NEE) all apply.  Shards, groups, canvas windows and external
 *                                   device buffers work unchanged.
 *   chunky_render_light_passes, chunky_render_adaptive*, chunky_render_robust_*   CHUNKY_E_STATE: not supported under fog.
 *   the first-hit passes (AOV, matte, occlusion), the preview and trace records   ignore fog: they see the world in clear air.
 * chunky_render_kernel_info's sixth word is 3 for a fog instantiation.  The Java binding does not reach these calls. */
typedef struct chunky_fog {
    size_t size;     /* sizeof(chunky_fog) of the caller */
    float density;   /* sigma >= 0 per block; 0 = off */
    float y_min, y_max;
    float color[3];  /* each in [0, 1] */
} chunky_fog;
int chunky_render_set_fog(chunky_render* r, const chunky_fog* fog);
int chunky_render_fog(chunky_render* r, chunky_fog* out);
int chunky_fog_check(const chunky_fog* fog);
/* self test (no device): plan_fog (csrc/launch_plan.hpp) for n rows of 8 ints {CHUNKY_OPT_KERNEL word, projector type, max depth, wide
 * tree (0 / 1), entity BVHs (0 / 1), BVH records (0 / 1), biome map applied (0 / 1), wide levels}; out8 per row {status, refusal, tree,
 * park, bvh, ext, family, 0}, and the refusal's text (NUL-terminated, at most 255 characters) in text256 per row when it is not NULL */
int chunky_selftest_plan_fog(const int32_t* rows8, int64_t n, int32_t* out8, char* text256);

/* Translucent blocks (no reference counterpart: K/material.h:50-54 tests a hit's alpha and drops it; arithmetic:
 * csrc/glass_spec.h; specification: tests/glass_port.c).
 *
 * Off by default: every hit whose alpha passes the reference's test is opaque.  With translucency on, a hit of colour c and alpha a
 * (after the tint multiply) with a < opaque_alpha is TRANSLUCENT for a ray that has crossed fewer than max_crossings such hits:
 *   the path's own ray draws one random number u: u < a, and the hit is a surface vertex as ever; otherwise the ray crosses — throughput
 *     *= (1 - a) + a c per channel, no emission, the depth unchanged — and is traced on in its direction from the far side;
 *   a shadow ray (towards the sun, or an emitter sample) draws nothing: its light is multiplied by (1 - a) ((1 - a) + a c) per channel
 *     and it goes on, clipped at what is left of its distance; an opaque hit, or a translucent one at the cap, blocks it as ever.
 * A ray that has crossed into a block of the octree is inside that block's RUN: it steps through every leaf of the same block without
 * a test — a lake or a glass wall is one interface, met on the way in — until it meets a leaf that cannot be hit (air).  A bounce and
 * the shadow rays of a vertex start inside the run the vertex was reached through.  No refraction, no absorption by path length.
 * With nothing translucent in view the image is the extended integrator's, bit for bit.
 *
 * chunky_render_set_translucency: `t` NULL turns the feature off; else t->size is the caller's sizeof(chunky_translucency) (a smaller
 * struct that still holds max_crossings is taken; a larger one when its extra bytes are all 0), opaque_alpha must lie in (0, 1]
 * (default 0.99: an alpha byte of 0xFF arrives as 255/256, or (255/256)^2 through a tint, and stays opaque) and max_crossings in
 * [1, 31] (default 8).  CHUNKY_E_INVALID, nothing changed, otherwise.  It touches no image and reaches every member of a group; like a
 * change of options it ends an adaptive run that could have been resumed.
 * chunky_render_translucency reports the parameters (out->size is set to this header's sizeof) and, in *enabled when not NULL, whether the
 * feature is on.  chunky_translucency_check is set_translucency's test without a target or a device.
 *
 * While translucency is on:
 *   chunky_render_passes            runs the glass kernels (the extended integrator whatever the light-transport options say, which all
 *                                   apply), or answers CHUNKY_E_STATE with the reason, before anything is launched or written: a fog
 *                                   layer on the target, and everything chunky_render_set_fog lists for fog.  Shards, groups, canvas
 *                                   windows and external device buffers work unchanged.
 *   chunky_render_light_passes, chunky_render_adaptive*, chunky_render_robust_*, chunky_render_set_fog with a density
 *                                   CHUNKY_E_STATE: not supported with translucent blocks.
 *   the first-hit passes (AOV, matte, occlusion), the preview and trace records   ignore it: every hit is opaque to them.
 * chunky_render_kernel_info's sixth word is 4 for a glass instantiation.  The Java binding does not reach these calls. */
typedef struct chunky_translucency {
    size_t size;           /* sizeof(chunky_translucency) of the caller */
    float opaque_alpha;    /* in (0, 1] */
    int32_t max_crossings; /* in [1, 31] */
} chunky_translucency;
int chunky_render_set_translucency(chunky_render* r, const chunky_translucency* t);
int chunky_render_translucency(chunky_render* r, chunky_translucency* out, int* enabled);
int chunky_translucency_check(const chunky_translucency* t);
/* self test (no device): plan_glass (csrc/launch_plan.hpp) for n rows of 9 ints {CHUNKY_OPT_KERNEL word, projector type, max depth, wide
 * tree (0 / 1), entity BVHs (0 / 1), BVH records (0 / 1), biome map applied (0 / 1), wide levels, fog layer (0 / 1)}; out8 per row
 * {status, refusal, tree, park, bvh, ext, family, words of a parked path}, and the refusal's text in text256 per row when it is not NULL */
int chunky_selftest_plan_glass(const int32_t* rows9, int64_t n, int32_t* out8, char* text256);

typedef enum chunky_option {
    CHUNKY_OPT_DRAW_DEPTH = 0,      /* int, default 256  (K/rayTracer.cl:94) */
    CHUNKY_OPT_MAX_DEPTH = 1,       /* int >= 1, default 5 (K/rayTracer.cl:107); above 254 the fallback kernels run (render_pool marks a
                                     * fresh path with depth 255), which have none of the extensions below: with any of them set,
                                     * chunky_render_passes then returns CHUNKY_E_STATE before it launches or writes anything */
    CHUNKY_OPT_EMITTER_SCALE = 2,   /* float bits, default 13.0f (K/rayTracer.cl:99) */
    CHUNKY_OPT_KERNEL = 3,          /* int: kernel variant, 0 = default (the pool kernel); bit 0 reference octree layout, bit 1
                                     * one lane per path (render_lanes), bit 2 phase profile (pool kernel), bit 3 the
                                     * fallback kernel render_waves instead of the pool kernel, bits 4-5 (render_waves)
                                     * lanes per pixel 1/8/16, bits 6-7 (pool kernel) paths parked per wave none/32 instead
                                     * of 64, bit 8 / bit 9 (pool kernel) full cubes and model blocks tested in phases of their own: always / never
                                     * (default: where model blocks are common, from 3 % of the world's leaves on) (all bit-identical) */
    /* EXPERIMENTAL light-transport extensions (the reference has none of them — it gates sun
     * sampling on drawTexture, PackedSun.java:16 / K/sky.h:69, ignores emittersEnabled, and loads material word 5 without
     * using it, K/material.h:38).  Specification: oracle/port.c trace_sample_ext; DESIGN.md section 9.  The defaults are the
     * reference's behaviour and run the reference kernels. */
    CHUNKY_OPT_SUN_SAMPLING = 4,    /* int: -1 as the reference (PackedSun flag bit 0), 0 never, 1 always (Chunky sunEnabled) */
    CHUNKY_OPT_EMITTERS = 5,        /* int: 1 (default) / 0 = Chunky emittersEnabled false */
    CHUNKY_OPT_BSDF = 6,            /* int: 0 (default) / 1 = specular, metalness, roughness from material word 5 (PackedMaterial.java:69-71) */
    CHUNKY_OPT_EMITTER_NEE = 7,     /* int: 0 (default) / 1 = next-event estimation towards the scene's emitter blocks */
    /* (The bounce ray that follows an emitter sample keeps the emittance of what it hits unless the emitter list holds it: the
     * emittance is dropped only when the octree part of the trace won (no entity triangle nearer), the block's model type is 1,
     * and its material has flag 2 clear and a non-zero emittance byte — chunky_scene_emitters' own condition.  Emissive model
     * blocks, cubes with an emittance texture and emissive entity triangles are not sampled, so they keep their implicit light.) */
    /* EXTENSION, not the reference's walk: 1 = in the entity-BVH traversal a child whose box lies entirely BEHIND the ray origin
     * (the far end of the slab test is negative) counts as missed.  The reference's quick test (K/primitives.h:30-48, used by
     * K/bvh.h:72-85) has no such exit: it descends into every box the ray's LINE pierces, and about half of its node visits and
     * triangle tests are spent behind the origin (EXPERIMENTS.md 4.4).  A triangle there can only be "hit" when rounding noise
     * carries its barycentric test across, and that DOES happen: with entity boxes on the block grid and a bounce origin within a
     * few ulps of a box edge, the reference accepts a hit the culled walk never tests — 40 of 10^8 adversarial traces
     * (EXPERIMENTS.md 5.3, tests/test_bvh_cull.py).  Whole frames are usually identical to the reference's, single pixels
     * occasionally not: hence an option, and 0 the default.  Specification: oracle/port.c with port_set_bvh_cull(1). */
    CHUNKY_OPT_BVH_CULL_BEHIND = 8, /* int: 0 (default) / 1 */
    /* 1 (default): a scene's biome map (chunky_scene_set_biome_tints) tints this target's images by block position; 0: the target
     * ignores the map and runs exactly the kernels it runs for a scene without one.  Without a map the option does nothing. */
    CHUNKY_OPT_BIOME_TINT = 9       /* int: 1 (default) / 0 */
} chunky_option;
int chunky_render_set_option(chunky_render* r, int option, int32_t value);

/* Multi-GPU image-tile ownership (no reference counterpart — the reference is single-device):
 * tile = 0: the image is cut into blocks of 16 x 16 pixels (row-major over blocks, edge blocks
 * partial), block b belongs to rank b % world — the shape the pool kernel renders in, so a share
 * runs as fast per pixel as the whole image (other kernels refuse it); tile > 0: pixel indices are
 * cut into runs of `tile` consecutive gids, run t belongs to rank t % world (every kernel).
 * A rank renders only its tiles; every other pixel of its buffer stays 0, so a SUM reduce over
 * ranks (one RCCL collective per read-back) reproduces the 1-GPU image bit for bit.
 * Any tile >= 0 and any 0 <= rank < world <= INT_MAX are taken.  A tile at or above the pixel count acts exactly as
 * tile = width * height (it is stored clamped): rank 0 owns every pixel, every other rank none.  A rank at or beyond the number of
 * tiles or blocks owns nothing: render, AOV, read and gather calls on it return CHUNKY_OK having done nothing.  CHUNKY_E_INVALID
 * for the one share whose slots do not fit an int: 16 x 16 blocks (256 slots each) of an image so thin that a rank's blocks hold
 * more than 2^31 slots (e.g. 1 x 2^30 pixels over 2 ranks). */
int chunky_render_set_shard(chunky_render* r, int rank, int world, int tile);
/* (On a group's render target the members split the caller's share again: member i of n renders as rank + world * i of world * n;
 * CHUNKY_E_INVALID, with no member changed, when world * n does not fit an int or a member's share is the one refused above.) */
/* Use a caller-owned device buffer (3*width*height floats) as the framebuffer, e.g. a torch tensor
 * that torch.distributed reduces over RCCL.  NULL returns to the internal buffer.
 * Ordering contract: the library runs on its own non-blocking stream and only synchronises THAT stream here.  The caller
 * must have completed every write of its own to the buffer (e.g. torch.zeros: torch.cuda.synchronize() first) before the
 * next chunky_render_passes, and must call chunky_render_sync before it reads or reduces the buffer on another stream. */
int chunky_render_set_device_buffer(chunky_render* r, void* device_ptr);
int chunky_render_device_buffer(chunky_render* r, void** device_ptr);
/* Zero the device framebuffer (the reference uploads a zeroed passBuffer, OpenClPathTracingRenderer.java:61,71). */
int chunky_render_reset(chunky_render* r);

/* Enqueue n passes: pass k uses seeds[k] as *randomSeed and first_buffer_spp + k as *bufferSpp
 * (OpenClPathTracingRenderer.java:106-141; n = 1 reproduces the reference's one launch per spp).
 * Asynchronous; chunky_render_sync / chunky_render_read wait. */
int chunky_render_passes(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp);
int chunky_render_sync(chunky_render* r);
/* Blocking read-back of the running-mean buffer, 3*width*height floats (clEnqueueReadBuffer,
 * OpenClPathTracingRenderer.java:164-166). */
int chunky_render_read(chunky_render* r, float* out, int64_t n_floats);
/* The exchange of chunky_render_read without the copy to the host: waits for the queued passes; on a group it then gathers
 * every member's blocks into member 0's device buffer (chunky_render_device_buffer), which holds the whole image afterwards.
 * On a single-device target it is chunky_render_sync. */
int chunky_render_gather(chunky_render* r);
/* Device time of the render kernels enqueued since the last call, from HIP events on the stream the
 * kernels run on: total milliseconds and number of launches. */
int chunky_render_kernel_time(chunky_render* r, float* total_ms, int* launches);
/* (On a group: the largest member total — the members run concurrently — and member 0's launch count.) */

/* Which kernel instantiation the most recent chunky_render_passes launch ran (no reference counterpart; the parity
 * tests assert it, so that a comparison with the oracle is a comparison of the kernel that is timed): out8 =
 * {tree form: 0 reference octree layout (K/octree.h:81-89), -1 generic wide tree, 16 + n dense top node over n levels
 * of 8x8x8 nodes; lanes per pixel (0 = one lane per pixel for the whole launch); entity-BVH phases present (K/bvh.h:22-113);
 * workgroups launched; paths parked per wave (pool kernel; -1 = the grouped kernel); extended integrator; the most passes one
 * launch of this target carries (256, fewer when the staged samples of a launch would not fit: chunky_render_passes cuts longer
 * requests into launches of that many); 1 when the launch tested full cubes and model blocks in phases of their own}.  On a group:
 * member 0's launch.  The sixth word is 2 for a biome-tint instantiation (chunky_scene_set_biome_tints), before the target's first launch
 * too: the first five words then name the instantiation its next launch will run (workgroups 0).  It is 3 for a ground-fog
 * instantiation (chunky_render_set_fog), likewise, and 4 for a translucent-blocks instantiation (chunky_render_set_translucency). */
int chunky_render_kernel_info(chunky_render* r, int32_t out8[8]);

/* Profile of the wave-scheduled kernel, filled only while CHUNKY_OPT_KERNEL has bit 2 set: for each of
 * the phases MARCH, BLOCK, SHADE the number of wave-level executions, the lanes active in them and
 * the shader cycles spent (s_memtime), summed over all waves since the last reset (9 values), then
 * the sum and the maximum of the wave lifetimes and the number of waves (3 values), then the executions
 * and cycles of the pixel/pass hand-over part of SHADE (2 values), then ten cycle sums of parts of SHADE
 * (sky lookup, direction sampling, trace setup, then the hand-over's deposit, fold, pixel opening, pass hand-out,
 * new sample; then, of the pool kernel's phase for model blocks — where it tests them apart from the full cubes, CHUNKY_OPT_KERNEL
 * bit 8 — lanes (executions in bits 40 up) and cycles): 24 values in all. */
int chunky_render_phase_stats(chunky_render* r, uint64_t* out24, int reset);
/* One more count of the same profile (pool kernel only): of the MARCH lanes counted above, the lane-steps taken at or above the
 * scene's hit_top (chunky_scene_hit_top) by a ray that runs upwards — steps that can find nothing.  Reset by either call. */
int chunky_render_march_above(chunky_render* r, uint64_t* out1, int reset);

/* Preview kernel (K/rayTracer.cl:115-217; OpenClPreviewRenderer.java:47-115): width*height ARGB ints. */
int chunky_render_preview(chunky_render* r, int32_t* argb_out);

/* Parity instrument: for each gid, the outcome of every closestIntersect of one sample (main and
 * shadow traces in call order) and the sample's radiance. */
typedef struct chunky_hit_record {
    int32_t hit;       /* closestIntersect result */
    int32_t material;  /* record.material: block-palette pointer of the octree hit */
    float distance;
    float normal[3];
    float color[4];
    float emittance;
    float point[3];
} chunky_hit_record;
#define CHUNKY_MAX_TRACES 10
int chunky_render_trace_records(chunky_render* r, int32_t seed, const int32_t* gids, int n,
                                chunky_hit_record* records /* n*CHUNKY_MAX_TRACES */, int32_t* counts /* n */,
                                float* radiance /* 3n */);

/* ---- auxiliary images for an external denoiser (no reference counterpart: Chunky's denoiser plugin traces them again on the
 * CPU for Open Image Denoise).  The albedo and the normal of the first surface each camera ray hits, averaged over passes.
 * Pass k of a call uses seeds[k] and bufferSpp first_buffer_spp + k exactly like chunky_render_passes; its sample at pixel gid
 * is the FIRST trace of that reference pass: RNG state seed + gid, Random_nextState, the camera ray (K/rayTracer.cl:55-91), one
 * closestIntersect with the target's draw depth and CHUNKY_OPT_BVH_CULL_BEHIND (K/kernel.h:14-24).  A hit gives albedo =
 * record.color.xyz before applyRayColor and normal = record.normal; a miss gives albedo = the sky colour of intersectSky with
 * record.emittance = 1 (the radiance of a reference sample whose first trace misses, K/rayTracer.cl:94-97) and normal = (0, 0, 0).
 * Each channel is folded in float, in pass order, with the running mean of K/rayTracer.cl:109-112.  So AOV pass k sees the camera
 * ray render pass k sees with the same seed: a host that passes the seeds of its first N render passes gets images that line up
 * with its beauty samples.  The other light-transport options and CHUNKY_OPT_MAX_DEPTH do not touch the first trace and are ignored.
 * The two images are allocated, zeroed, by the first AOV call on a target; chunky_render_reset / _read / _kernel_time /
 * _kernel_info never see them, nor AOV launches.  A set shard (chunky_render_set_shard) limits the passes to the rank's pixels; the
 * others stay 0.  On a group's render target member 0 renders the caller's whole share (as chunky_render_preview does): the
 * images are the one-context images, with no exchange. */
#define CHUNKY_AOV_ALBEDO 0
#define CHUNKY_AOV_NORMAL 1
/* Enqueue n AOV passes (asynchronous, like chunky_render_passes; longer requests are cut into launches of at most 256 passes,
 * which changes no bit).  CHUNKY_E_STATE before chunky_render_set_camera.  A ground-fog layer (chunky_render_set_fog) is ignored:
 * the images are of the world in clear air. */
int chunky_render_aov_passes(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp);
/* Blocking read-back of one image (which = CHUNKY_AOV_ALBEDO or CHUNKY_AOV_NORMAL), 3*width*height floats, like
 * chunky_render_read.  CHUNKY_E_STATE before any AOV pass. */
int chunky_render_aov_read(chunky_render* r, int which, float* out, int64_t n_floats);
/* Zero both images (chunky_render_reset for the AOV). */
int chunky_render_aov_reset(chunky_render* r);
/* Device time of the AOV launches enqueued since the last call, from HIP events on the stream they run on (as
 * chunky_render_kernel_time). */
int chunky_render_aov_kernel_time(chunky_render* r, float* total_ms, int* launches);
/* The AOV instantiation the most recent launch ran (as chunky_render_kernel_info): out4 = {tree form (0 reference octree layout,
 * -1 generic wide tree, 16 + n dense top node over n levels: the form render_pool runs for the scene), entity-BVH walk present,
 * workgroups launched, launches made by the most recent chunky_render_aov_passes}.  Bit 1 of the second word: a biome-tint instantiation
 * (chunky_scene_set_biome_tints). */
int chunky_render_aov_kernel_info(chunky_render* r, int32_t out4[4]);

/* ---- five more images of the same first hit, for compositing: coverage ("transparent sky"), depth, position, emittance and the
 * block hit.  The sample is exactly the AOV sample above, and `rec` is record 0 of chunky_render_trace_records for it:
 *
 *   image                  words per pixel   sample on a hit                       on a miss
 *   CHUNKY_AOV_ALPHA       1 float           1.0f                                  0.0f
 *   CHUNKY_AOV_DEPTH       1 float           rec.distance                          0.0f
 *   CHUNKY_AOV_POSITION    3 floats          rec.point = o + d * (distance - OFFSET)   (0, 0, 0)
 *   CHUNKY_AOV_EMITTANCE   1 float           rec.emittance                         0.0f
 *   CHUNKY_AOV_BLOCK       1 int32           rec.material                          -1
 *
 * The four float images are folded like albedo and normal: (img * spp + v) / (spp + 1) in float, in pass order.  A miss folds a 0,
 * so DEPTH, POSITION and EMITTANCE are hit-weighted sums over the passes, divided by the pass count: the mean over the samples
 * that hit is image / ALPHA (where ALPHA > 0).  BLOCK is not averaged: every pass overwrites it, so it holds the value of the last
 * pass folded.  For antialiased masks use the ID mattes below (chunky_render_matte_passes), which count every pass's id per pixel.
 * DEPTH is the reference's ray parameter t of the hit (hit = o + d * t), so its unit is the length of the camera ray's direction d:
 *  - the projected cameras (CHUNKY_PROJ_PARALLEL .. CHUNKY_PROJ_ODS_STACKED, with or without a lens) normalise d: DEPTH is the
 *    distance from the ray's origin in blocks (to float rounding, and given the orthonormal matrix a camera has);
 *  - the pinhole camera (type 0) does not (K/camera.h:19): without a lens d = m * (fovTan x, fovTan y, 1), so DEPTH is the depth
 *    along the view axis (planar z), not the distance; with a lens (aperture > 0) d's view-axis component is subjectDistance, and
 *    DEPTH * subjectDistance is that planar depth;
 *  - pre-generated rays (type -1) have the length their table gives them.
 * POSITION is in world units (blocks, octree coordinates) for every camera.
 * BLOCK is rec.material: for a block hit, the octree leaf's value for that block (its offset in the block palette, K/octree.h:88).
 * The entity BVHs never write that field (K/bvh.h), so for an entity hit it is what the octree part of the same trace left there:
 * the block the ray would have hit behind the entity, or 0 where the octree missed.
 * chunky_render_aov_passes_ex folds all seven images (albedo, normal and these five) from one trace per sample; albedo and normal
 * after it are, bit for bit, what chunky_render_aov_passes gives with the same arguments.  The five images are allocated, zeroed, by
 * the first _ex call on a target, and chunky_render_aov_reset zeroes them too where they exist.  chunky_render_aov_passes never
 * touches them: a host that mixes the two calls lets the five images lag behind albedo and normal.  Shards and groups as for the
 * AOV; chunky_render_aov_kernel_time / _kernel_info cover _ex launches as they cover AOV launches. */
#define CHUNKY_AOV_ALPHA 2
#define CHUNKY_AOV_DEPTH 3
#define CHUNKY_AOV_POSITION 4
#define CHUNKY_AOV_EMITTANCE 5
#define CHUNKY_AOV_BLOCK 6
/* Enqueue n passes over all seven images (asynchronous; cut into launches of at most 256 passes, which changes no bit).
 * CHUNKY_E_STATE before chunky_render_set_camera.  A ground-fog layer (chunky_render_set_fog) is ignored. */
int chunky_render_aov_passes_ex(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp);
/* Blocking read-back of one image, which = CHUNKY_AOV_ALBEDO .. CHUNKY_AOV_BLOCK; n_words = width*height times the words per pixel
 * of the image (3 for albedo, normal and position, else 1; floats, int32 for CHUNKY_AOV_BLOCK).  CHUNKY_E_STATE before the first
 * _ex pass for which >= CHUNKY_AOV_ALPHA (before any AOV pass for the other two); CHUNKY_E_INVALID for an unknown image or a
 * wrong count. */
int chunky_render_aov_read_ex(chunky_render* r, int which, void* out, int64_t n_words);

/* ---- two images of the light at that first surface, from the beauty sample's own rays: how much of the sun the surface sees, and how
 * open it is to its surroundings (ambient occlusion).  The sample of pass k at pixel gid is the reference's pass-k sample cut off
 * after its first bounce trace: RNG state seeds[k] + gid, Random_nextState, the camera ray of the target's camera (with its aperture
 * or lens), then up to three closestIntersect calls, each with the target's draw depth and CHUNKY_OPT_BVH_CULL_BEHIND.  rec[i] is
 * record i of chunky_render_trace_records for that (seed, gid); `sun` is bit 0 of the PackedSun flags of the scene:
 *
 *   image            words per pixel   first trace misses   first trace hits
 *   CHUNKY_AOV_SUN   1 float           1.0f                 sun ? (rec[1].hit ? 0 : 1) : 0
 *   CHUNKY_AOV_AO    1 float           1.0f                 with b = rec[sun ? 2 : 1]: (b.hit && b.distance < ao_distance) ? 0 : 1
 *
 * Both are folded like the AOV: (img * spp + v) / (spp + 1) in float, in pass order, spp = first_buffer_spp + k.  A miss folds 1 — a
 * sky pixel is neither shadowed nor occluded — so either image multiplies straight over the beauty image and antialiased silhouettes
 * come out right; the mean over the samples that hit is (image - (1 - ALPHA)) / ALPHA with the coverage CHUNKY_AOV_ALPHA of
 * chunky_render_aov_passes_ex over the same seeds (where ALPHA > 0).
 * The sun trace is the reference's (K/rayTracer.cl:101-106), quirks included: direction normalize(u * v + w) (K/sky.h:86), origin
 * rec[0].point with no offset, and its record is a copy of the first hit's, distance included, so only occluders nearer than the first
 * hit count.  SUN is therefore "the shadow the beauty image has", not a geometric visibility.  With the sun flag off there is no sun
 * ray and no RNG draw for it: SUN folds 0 on hits, and the bounce uses the two draws right after the camera's, as the reference does.
 * The pass follows the scene's sun flag (chunky_scene_set_sun), not CHUNKY_OPT_SUN_SAMPLING; CHUNKY_OPT_MAX_DEPTH and the
 * experimental light-transport options are ignored, as for the AOV.
 * The bounce trace is nextPath's (K/kernel.h:46-98): one cosine-weighted direction about rec[0].normal, origin rec[0].point + d *
 * OFFSET, the record's distance reset to +inf — so AO is the usual cosine-weighted estimator, "the share of bounce rays that meet
 * nothing within ao_distance".  `b.distance < ao_distance` is one strict float compare: a negative distance (which occurs) counts as
 * occluded, a NaN distance as clear.  ao_distance is in the unit of the bounce direction (a unit vector to float rounding: blocks),
 * > 0, and +inf is allowed: AO is then the share of bounce rays that reach the sky.
 * The two images are allocated, zeroed, by the first chunky_render_occlusion_passes on a target.  Render, AOV, matte, denoise and
 * adaptive calls never see them (chunky_render_aov_reset does not touch them), and these calls never touch theirs.  A set shard limits
 * the passes to the rank's pixels; the others stay 0.  On a group's render target member 0 renders the caller's whole share, as for
 * the AOV.  A scene update between two calls (chunky_scene_set_sun, ...) takes effect in the next one.  The Java binding does not
 * reach these calls. */
#define CHUNKY_AOV_AO 7
#define CHUNKY_AOV_SUN 8
/* Enqueue n passes over both images (asynchronous; cut into launches of at most 256 passes, which changes no bit; n = 0 is legal).
 * CHUNKY_E_STATE before chunky_render_set_camera; CHUNKY_E_INVALID for ao_distance zero, negative or NaN.  A ground-fog layer
 * (chunky_render_set_fog) is ignored: both images are of the world in clear air. */
int chunky_render_occlusion_passes(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp, float ao_distance);
/* Blocking read-back of one image (which = CHUNKY_AOV_AO or CHUNKY_AOV_SUN), width*height floats.  CHUNKY_E_STATE before the first
 * chunky_render_occlusion_passes; CHUNKY_E_INVALID for an unknown image or a wrong count. */
int chunky_render_occlusion_read(chunky_render* r, int which, float* out, int64_t n_floats);
/* Zero both images. */
int chunky_render_occlusion_reset(chunky_render* r);
/* Device time of the occlusion launches enqueued since the last call (as chunky_render_aov_kernel_time; no other timer sees them). */
int chunky_render_occlusion_kernel_time(chunky_render* r, float* total_ms, int* launches);
/* The instantiation the most recent occlusion launch ran: the four words of chunky_render_aov_kernel_info. */
int chunky_render_occlusion_kernel_info(chunky_render* r, int32_t out4[4]);

/* ---- light groups: the sky's, the sun's and the emitters' share of the beauty image as images of their own, so that a compositor
 * rebalances the three ("torches warmer, sun down a stop") with a weighted sum of finished images instead of a new render.  The
 * sample of pass k at pixel gid is the reference's whole sample (K/rayTracer.cl:55-107): RNG state seeds[k] + gid,
 * Random_nextState, the camera ray of the target's camera (with its aperture or lens), then the traces, the sun rays (bit 0 of the
 * scene's PackedSun flags) and the bounces up to CHUNKY_OPT_MAX_DEPTH, each trace with the target's draw depth and
 * CHUNKY_OPT_BVH_CULL_BEHIND.  Its radiance is a sum of terms linear in three scalars, and each image evaluates them with a triple
 * of its own:
 *
 *   image                   sky intensity   sun intensity (PackedSun word 3)   emitter scale (CHUNKY_OPT_EMITTER_SCALE)
 *   CHUNKY_LIGHT_SKY        the scene's     0                                  0
 *   CHUNKY_LIGHT_SUN        0               the scene's                        0
 *   CHUNKY_LIGHT_EMITTERS   0               0                                  the target's
 *   CHUNKY_LIGHT_ALL        the scene's     the scene's                        the target's
 *
 * A group image IS the reference's image under those scalars, bit for bit; the path itself never depends on them and is walked
 * once.  Per group, in the reference's operation order: at a hit, radiance += (c * (emittance * scale)) * throughput; at a miss or
 * an unshadowed sun ray, c = blend * sky (blend: the weighted sum of the four sky texels), then c += texel * sun where the direction
 * is in the sun's disc, then radiance += (c * throughput) * e.  CHUNKY_LIGHT_ALL is the beauty sample itself: the image
 * chunky_render_passes folds for the same seeds.  The three groups sum to it to rounding (at one pass, within
 * 4 * (2 * max depth + 3) * 2^-24 relative per float), and a doubled scalar doubles its group bit for bit.  With the sun flag off
 * there is no sun ray and no RNG draw for it, and CHUNKY_LIGHT_SUN is all zero.
 * Each image (3 floats per pixel, interleaved like the beauty image) is folded with (img * spp + v) / (spp + 1) in float, in pass
 * order, spp = first_buffer_spp + k.  The four images are allocated, zeroed, by the first chunky_render_light_passes on a target.
 * Render, AOV, matte, occlusion, denoise and adaptive calls never see them, and these calls never touch theirs.  A set shard limits
 * the passes to the rank's pixels; the others stay 0.  On a group's render target member 0 renders the caller's whole share, as for
 * the AOV.  A scene update between two calls (chunky_scene_set_sky, chunky_scene_set_sun, ...) takes effect in the next one.
 * The experimental light-transport options (CHUNKY_OPT_SUN_SAMPLING, CHUNKY_OPT_EMITTERS, CHUNKY_OPT_BSDF, CHUNKY_OPT_EMITTER_NEE)
 * change what the beauty image is; this pass does not implement them and refuses to run with any of them away from its default.
 * The Java binding does not reach these calls. */
#define CHUNKY_LIGHT_SKY 0
#define CHUNKY_LIGHT_SUN 1
#define CHUNKY_LIGHT_EMITTERS 2
#define CHUNKY_LIGHT_ALL 3
/* Enqueue n passes over the four images (asynchronous; cut into launches of at most 256 passes, which changes no bit; n = 0 is
 * legal).  CHUNKY_E_STATE before chunky_render_set_camera, with an experimental light-transport option set, and while the target
 * has a ground-fog layer (chunky_render_set_fog). */
int chunky_render_light_passes(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp);
/* Blocking read-back of one image (which = CHUNKY_LIGHT_SKY .. CHUNKY_LIGHT_ALL), 3*width*height floats.  CHUNKY_E_STATE before the
 * first chunky_render_light_passes; CHUNKY_E_INVALID for an unknown image or a wrong count. */
int chunky_render_light_read(chunky_render* r, int which, float* out, int64_t n_floats);
/* A rebalanced image on the device, read back: out = (w[0] * SKY + w[1] * SUN) + w[2] * EMITTERS per float, in that order, each
 * operation rounded to float (no fma); 3*width*height floats, ready for chunky_filter_frame once widened to double.
 * CHUNKY_E_INVALID for NULL or non-finite weights, a NULL buffer or a wrong count; CHUNKY_E_STATE before the first
 * chunky_render_light_passes (there is nothing to mix). */
int chunky_render_light_mix(chunky_render* r, const float w[3], float* out, int64_t n_floats);
/* Zero the four images. */
int chunky_render_light_reset(chunky_render* r);
/* Device time of the light-group launches enqueued since the last call (as chunky_render_aov_kernel_time; no other timer sees them). */
int chunky_render_light_kernel_time(chunky_render* r, float* total_ms, int* launches);
/* The instantiation the most recent light-group launch ran: the four words of chunky_render_aov_kernel_info. */
int chunky_render_light_kernel_info(chunky_render* r, int32_t out4[4]);

/* ---- emitter light groups: CHUNKY_LIGHT_EMITTERS split by what emits, so that a compositor turns the torches down while the lava
 * stays.  Ids are the ids of the ID mattes below: a block pointer (rec.material of an octree hit: even, >= 0, inside the block
 * palette), CHUNKY_MATTE_WORLD_ENTITY or CHUNKY_MATTE_ACTOR_ENTITY; the id of a hit names the last part of closestIntersect that
 * won, at every vertex of the path, not only the first.  Every id belongs to one of n_groups groups; an id that is not listed
 * belongs to group 0, "the rest".
 *
 * Specification.  For group g take the scene in which every block and entity triangle whose id is NOT in g keeps its place but
 * points to copies of its materials with bit 1 of word 0 cleared and word 4 zero (the emittance becomes exactly 0).  Group g's image
 * IS the reference's image of that scene with sky intensity 0, sun intensity 0 and the target's emitter scale, bit for bit.  Per
 * sample the group's sum receives, in vertex order, the (c * (emittance * scale)) * throughput that CHUNKY_LIGHT_EMITTERS receives at
 * the hits whose id maps to g, and at every miss or unshadowed sun ray the same literally evaluated (dark * throughput) * e term
 * (a NaN direction makes every group NaN, as it does the reference).  A hit of another group adds (c * (0 * scale)) * throughput,
 * which is +-0 for a finite scale and changes no sum: a sum that starts at +0 is never -0.  Each group image folds with
 * (img * spp + v) / (spp + 1) every pass, also where v is +0.  The groups sum to CHUNKY_LIGHT_EMITTERS to rounding (at one pass
 * within the bound above).
 *
 * With groups set, chunky_render_light_passes folds the four images exactly as before, bit for bit, and one image per group from
 * the same walk; shards, group targets, chunky_render_light_reset (which zeroes the group images too), _kernel_time and _kernel_info
 * (bit 2 of word 1: the kernel that carries the groups ran) behave as for the four images, and so do the refusals (the experimental
 * light-transport options, a biome-tinted target).  A scene update that shortens the block palette afterwards is legal: a pointer
 * beyond the stored table is group 0.  The Java binding does not reach these calls. */
#define CHUNKY_LIGHT_MAX_EMITTER_GROUPS 8
/* Set (n_groups 1 .. 8) or drop (n_groups 0, which frees the group images: every light call then behaves exactly as without this
 * call) the groups of a target: ids[i] belongs to group_of[i] < n_groups.  The group images, allocated here, start at zero; the four
 * images are NOT touched, so the group images lag behind them unless the host calls chunky_render_light_reset too.  Waits for the
 * target's enqueued work.  CHUNKY_E_INVALID (nothing changes): n_groups outside 0 .. 8, n_ids < 0, NULL with n_ids > 0, ids with
 * n_groups 0, an odd pointer or one beyond the palette, any other negative id, an id listed twice, a group >= n_groups.  While groups
 * are set chunky_render_light_passes answers CHUNKY_E_STATE to a non-finite CHUNKY_OPT_EMITTER_SCALE (0 * inf would make the
 * specification NaN wherever another group is hit). */
int chunky_render_light_set_emitter_groups(chunky_render* r, int n_groups, const int32_t* ids, const uint8_t* group_of, int n_ids);
/* Blocking read-back of one group image, 3*width*height floats.  CHUNKY_E_STATE with no groups set or before the first
 * chunky_render_light_passes since they were set; CHUNKY_E_INVALID for a group outside 0 .. n_groups - 1 or a wrong count. */
int chunky_render_light_read_group(chunky_render* r, int group, float* out, int64_t n_floats);
/* A rebalanced image on the device, read back: out = ((w_sky * SKY + w_sun * SUN) + w_groups[0] * G0) + w_groups[1] * G1 ... per
 * float, in that order, each operation rounded to float (no fma).  n_groups must be the target's.  CHUNKY_E_INVALID for NULL or
 * non-finite weights, another n_groups, a NULL buffer or a wrong count; CHUNKY_E_STATE as chunky_render_light_read_group. */
int chunky_render_light_mix_groups(chunky_render* r, float w_sky, float w_sun, const float* w_groups, int n_groups, float* out, int64_t n_floats);

/* ---- antialiased ID mattes (no reference counterpart; the idea of Cryptomatte): per pixel a short list of (id, the number of passes
 * that saw it), counted over the same camera rays the beauty passes use, so that a mask for any set of ids is a sum of shares and
 * lines up with the antialiased image.  The exact arithmetic is chunkyclplugin_amd/csrc/matte_spec.h, which the kernels and the
 * chunky_matte_host_* twins both compile: counts are integers, and the result does not depend on how the passes are cut into calls
 * or launches.
 *
 * The sample of pass k at pixel gid is exactly the AOV sample above: seeds[k], RNG state seed + gid advanced once, the camera ray
 * of the target's camera (with its aperture or lens), one closestIntersect with the target's draw depth and
 * CHUNKY_OPT_BVH_CULL_BEHIND.  closestIntersect runs the octree, then the world BVH, then the actor BVH, and a later part wins only
 * with a strictly smaller distance.  The id of the sample names the last part that won:
 *
 *   nothing hit                      CHUNKY_MATTE_SKY
 *   the octree's block stands        rec.material (>= 0: the block's offset in the block palette, as CHUNKY_AOV_BLOCK for a block hit)
 *   a world-BVH triangle won         CHUNKY_MATTE_WORLD_ENTITY
 *   an actor-BVH triangle won        CHUNKY_MATTE_ACTOR_ENTITY
 *
 * (Unlike CHUNKY_AOV_BLOCK, an entity hit never reports the block behind it.)
 *
 * A pixel's state is CHUNKY_MATTE_SLOTS slots of (int32 id, int32 count) and one int32 `other`: 13 words, 52 bytes.  A slot with
 * count 0 is empty.  A sample with id v goes to the first occupied slot that holds v (count + 1), else to the first empty slot
 * (id = v, count = 1), else to `other` (+ 1).  Slots fill in arrival order and are never evicted; passes apply in call order; the sky
 * takes a slot like any id; the counts of a pixel and its `other` add up to the passes folded into it.  The passes on a target since
 * its last reset may not exceed 2^31 - 1.
 *
 * Layout: `ids` and `counts` are plane-major — slot (or rank) s of pixel gid is at [s * n_pixels + gid], six images each, with
 * n_pixels = width * height; `other`, a mask and every other per-pixel array hold one word per pixel.
 *
 * The planes are allocated, zeroed, by the first matte call on a target.  The render, AOV, denoise and adaptive calls never see them
 * and the matte calls never see theirs.  A set shard limits the passes to the rank's pixels; the others stay empty.  On a group's
 * render target member 0 renders the caller's whole share, as for the AOV.  The Java binding does not reach these calls. */
#define CHUNKY_MATTE_SLOTS 6
#define CHUNKY_MATTE_SKY (-1)
#define CHUNKY_MATTE_WORLD_ENTITY (-2)
#define CHUNKY_MATTE_ACTOR_ENTITY (-3)
#define CHUNKY_MATTE_EMPTY INT32_MIN
/* Enqueue n matte passes (asynchronous, like chunky_render_aov_passes; cut into launches of at most 256 passes, which changes no
 * word).  CHUNKY_E_STATE before chunky_render_set_camera; CHUNKY_E_INVALID, before any launch, when the target's passes would
 * exceed 2^31 - 1.  A ground-fog layer (chunky_render_set_fog) is ignored. */
int chunky_render_matte_passes(chunky_render* r, const int32_t* seeds, int n);
/* Empty every slot and set the pass count to 0. */
int chunky_render_matte_reset(chunky_render* r);
/* Blocking read-back of the state: ids and counts 6 * n_pixels words each, other n_pixels, *passes the passes since the last reset.
 * Waits for the queued passes.  CHUNKY_E_INVALID for a null pointer or n_pixels != width * height. */
int chunky_render_matte_read(chunky_render* r, int32_t* ids, int32_t* counts, int32_t* other, int64_t n_pixels, int32_t* passes);
/* Replace the state with one read earlier (a resumed render).  The state is checked with chunky_matte_state_check first:
 * CHUNKY_E_INVALID, and nothing changed, when it fails. */
int chunky_render_matte_restore(chunky_render* r, const int32_t* ids, const int32_t* counts, const int32_t* other, int64_t n_pixels,
                                int32_t passes);
/* The read-out for a Cryptomatte-style export: per pixel the slots by count descending, ties by the lower slot index.  Rank j gets
 * ids[j * n_pixels + gid] and coverage[...] = (float)count / (float)passes (each conversion rounds to nearest; one division); empty
 * slots come last with CHUNKY_MATTE_EMPTY and 0.0f, so a pixel outside the target's shard reads as six empty ranks.  Computed on the
 * device; waits for the queued passes.  CHUNKY_E_STATE while the target has no pass; CHUNKY_E_INVALID as chunky_render_matte_read. */
int chunky_render_matte_ranks(chunky_render* r, int32_t* ids, float* coverage, int64_t n_pixels);
/* A mask for a set of ids (any order; duplicates count once; n_set = 0 is the empty set): out[gid] = (float)(the sum of the counts
 * of the pixel's occupied slots whose id is in the set) / (float)passes — an integer sum and one division.  `other` is attributed to
 * no id: where it is not 0 (chunky_render_matte_read) masks undercount.  out has the layout chunky_filter_frame_alpha takes as
 * alpha.  Computed on the device; waits for the queued passes.  CHUNKY_E_STATE while the target has no pass; CHUNKY_E_INVALID for
 * n_set < 0, a null pointer, a wrong n_pixels or CHUNKY_MATTE_EMPTY in the set. */
int chunky_render_matte_extract(chunky_render* r, const int32_t* set, int n_set, float* out, int64_t n_pixels);
/* Device time of the matte-pass launches enqueued since the last call (as chunky_render_aov_kernel_time; the AOV's timer does not
 * see them, nor this one the AOV's). */
int chunky_render_matte_kernel_time(chunky_render* r, float* total_ms, int* launches);
/* The instantiation the most recent matte launch ran: the four words of chunky_render_aov_kernel_info. */
int chunky_render_matte_kernel_info(chunky_render* r, int32_t out4[4]);
/* The same arithmetic on the host (plain C++, no device needed), on states in the layout above.
 * _host_fold continues the state passed in with n_passes samples per pixel, sample_ids[pass * n_pixels + gid], in pass order.
 * _host_ranks and _host_extract are chunky_render_matte_ranks / _extract of a state after `passes` passes.  CHUNKY_E_INVALID for
 * null pointers, n_pixels <= 0, passes <= 0 (ranks, extract), negative counts, counts that add up to more than `passes` (or, for the
 * fold, that would pass 2^31 - 1), and CHUNKY_MATTE_EMPTY as a sample's id or in the set. */
int chunky_matte_host_fold(const int32_t* sample_ids, int n_passes, int64_t n_pixels, int32_t* ids, int32_t* counts, int32_t* other);
int chunky_matte_host_ranks(const int32_t* ids, const int32_t* counts, int64_t n_pixels, int32_t passes, int32_t* out_ids,
                            float* out_coverage);
int chunky_matte_host_extract(const int32_t* ids, const int32_t* counts, int64_t n_pixels, int32_t passes, const int32_t* set, int n_set,
                              float* out);
/* CHUNKY_OK when the state is one the fold can have left after `passes` passes (passes >= 0), else CHUNKY_E_INVALID with the rule
 * in chunky_last_error: counts >= 0 and other >= 0; a pixel's occupied slots contiguous from slot 0; no id twice among them; no
 * CHUNKY_MATTE_EMPTY in an occupied slot; per pixel the counts and `other` add up to 0 (a pixel outside the shard) or to passes. */
int chunky_matte_state_check(const int32_t* ids, const int32_t* counts, const int32_t* other, int64_t n_pixels, int32_t passes);

/* ---- denoising (no reference counterpart): an edge-avoiding À-Trous wavelet filter (Dammertz et al. 2010) guided by the albedo
 * and normal images above.  Closed-form and deterministic; the exact arithmetic is chunkyclplugin_amd/csrc/denoise_spec.h, which the
 * kernels and chunky_denoise_host both compile, so the device result equals the host's bit for bit.
 * Per pixel, colour C, albedo A, normal N (3 floats each, interleaved as chunky_render_read / chunky_render_aov_read deliver them),
 * m = max(A, 2^-10) per channel:
 *   D0 = C / m with CHUNKY_DENOISE_DEMODULATE, else C (a pure-sky pixel, whose albedo is its radiance, demodulates to about 1);
 *   iteration i = 0 .. iterations-1, step s = 1 << i: taps q = p + s (dx, dy), dy = -2..2 outer, dx = -2..2 inner, those outside
 *     the image skipped; h = k[|dx|] k[|dy|], k = {3/8, 1/4, 1/16}; dc, dn, da = sums over channels of the squared differences of
 *     D, N, A between q and p; x = (dc c_i + dn c_n) + da c_a with c_i = 4^i / sigma_color^2 (the colour sigma halves per
 *     iteration), c_n = 1 / sigma_normal^2, c_a = 1 / sigma_albedo^2, computed once in float; w = h e^(-x);
 *     D'(p) = (sum w D(q)) / (sum w), each sum in tap order;
 *   out = D m with CHUNKY_DENOISE_DEMODULATE.
 * Non-finite values do not spread: a tap whose D has a non-finite channel, or whose x is not finite, has weight 0; a pixel whose D
 * is non-finite, or whose weights sum to 0, keeps its D; a pixel whose input colour has a non-finite channel comes back as that
 * input colour.  albedo = 0 is legal (that is what the 2^-10 is for). */
#define CHUNKY_DENOISE_DEMODULATE 1u    /* flags bit 0 */
/* flags bits 8-9: how the kernels fetch their taps (no effect on the result or on chunky_denoise_host): 0 the default (the three
 * images read as they are, 3 floats per pixel), 1 the packed form (16-byte words per pixel written by a pack pass; measured slower) */
#define CHUNKY_DENOISE_KERNEL_SHIFT 8
#define CHUNKY_DENOISE_KERNEL_MASK 0x300u
typedef struct chunky_denoise_params {
    size_t size;          /* sizeof(chunky_denoise_params) as the CALLER was compiled (as chunky_run_callbacks::struct_size): members
                           * are appended over time and the library reads only those the caller's struct holds */
    int32_t iterations;   /* 1 .. 8 */
    float sigma_color;    /* finite and > 0, also the next two */
    float sigma_normal;
    float sigma_albedo;
    uint32_t flags;       /* CHUNKY_DENOISE_* ; unknown bits are CHUNKY_E_INVALID */
} chunky_denoise_params;
/* Fills *p with the defaults (5 iterations, demodulation on) and p->size with this library's struct size. */
int chunky_denoise_default_params(chunky_denoise_params* p);
/* The filter on the host, threaded over rows; takes no context and uses no device.  color / albedo / normal / out: 3*width*height
 * floats; out may not overlap an input.  This function is the specification the device entry points are held to.
 * CHUNKY_E_INVALID: a NULL pointer, width or height <= 0, size smaller than the first version of the struct (through `flags`),
 * iterations outside 1 .. 8, a sigma that is not finite or <= 0 (or so small or large that its coefficient is not a positive
 * finite float).  Images of 1 x 1, 1 x N and N x 1 are legal. */
int chunky_denoise_host(int width, int height, const float* color, const float* albedo, const float* normal,
                        const chunky_denoise_params* params, float* out);
/* The same on the device: uploads the three images, filters, reads the result back (blocking).  What a host calls on its merged
 * image after several read-backs.  Same validation. */
int chunky_denoise_frame(chunky_ctx* ctx, int width, int height, const float* color, const float* albedo, const float* normal,
                         const chunky_denoise_params* params, float* out);
/* Filters the target's own framebuffer with the target's own AOV images, all resident on the device; only the result crosses to the
 * host (out: n_floats = 3*width*height).  The framebuffer and the AOV images are read, never written: chunky_render_read /
 * chunky_render_aov_read return afterwards what they returned before.  Waits for the queued passes; on a group it runs on member 0
 * after the exchange of chunky_render_read.  CHUNKY_E_STATE before any AOV pass, and on a target whose shard
 * (chunky_render_set_shard with world > 1) does not hold the whole image. */
int chunky_render_denoise(chunky_render* r, const chunky_denoise_params* params, float* out, int64_t n_floats);
/* Device time of the denoise launches since the last call, from HIP events on the stream they run on (as
 * chunky_render_aov_kernel_time), and their number: one per iteration, plus one for the demodulation (or pack) pass. */
int chunky_render_denoise_kernel_time(chunky_render* r, float* total_ms, int* launches);
/* The filter's e^(-x) (x >= 0) evaluated on the host for n values: the instrument of its accuracy test. */
int chunky_denoise_exp(const float* x, int n, float* out);

/* ---- adaptive sampling: pixels stop when their noise estimate falls under a threshold; the rest are rendered from a list ----
 * No counterpart in the reference (it renders every pass on every pixel).  The arithmetic is chunkyclplugin_amd/csrc/adaptive_spec.h,
 * compiled by the kernels and the host alike; every operation is ONE exactly rounded float operation, no multiply-add is fused.
 *
 * State per pixel: n_p, the passes folded so far; the running-mean colour (the framebuffer, folded as K/rayTracer.cl:109-112:
 * mean = (mean * (float)k + c) / (float)(k + 1)); a Welford pair (m, M2) on luminance, both 0 at the start.
 *
 * Update for the sample c = (r, g, b) of pass k (k counted from 0, passes taken in order):
 *     y  = (r * 0.2126f + g * 0.7152f) + b * 0.0722f
 *     d  = y - m
 *     m  = m + d / (float)(k + 1)
 *     M2 = M2 + d * (y - m)                                    (the m just updated)
 *
 * Convergence test, applied only after n = min_spp + j * check_interval passes (j = 0, 1, ...) while n < max_spp (a check after
 * the last pass would change no result and is not run):
 *     b   = m > floor ? m : floor
 *     lim = ((t2 * ((float)n * (float)(n - 1))) * b) * b       with t2 = threshold * threshold, one float product made on the host
 *     the pixel is UNCONVERGED iff it is active and M2 > lim.
 * A pixel whose m or M2 is not finite (NaN or infinite) is converged: one bad pixel cannot hold a frame to max_spp.  The test reads
 * "relative standard error of the mean luminance > threshold": M2 / (n (n - 1)) is the variance of the mean.
 *
 * Activity: all pixels start active.  At a check a pixel stays active iff it was active and some pixel of its 3 x 3 neighbourhood,
 * clipped to the image, is unconverged (inactive pixels are never unconverged).  An inactive pixel never becomes active again, so
 * every active pixel has seen exactly the passes rendered so far.  A pixel that leaves at the check after n passes records n_p = n;
 * pixels still active after max_spp passes record max_spp.
 *
 * Result: pixel p of the framebuffer is, bit for bit, pixel p of chunky_render_passes(seeds[0 .. n_p), first_buffer_spp = 0) from a
 * reset target; count[p] = n_p; (m, M2)[p] is the Welford state after n_p samples.
 *
 * threshold = 0 renders max_spp passes wherever M2 > 0 (a pixel with M2 == 0, e.g. a constant one, converges at the first check). */
typedef struct chunky_adaptive_params {
    size_t size;            /* sizeof(chunky_adaptive_params) as the caller was compiled (members may be appended) */
    float threshold;        /* finite, >= 0: relative standard error of the mean luminance under which a pixel is converged */
    float floor;            /* finite, > 0: the least luminance the error is taken relative to (dark pixels) */
    int32_t min_spp;        /* >= 2: passes before the first check */
    int32_t check_interval; /* >= 1: passes between checks */
    uint32_t flags;         /* no bit is defined yet: must be 0 */
    uint32_t reserved;      /* ignored */
} chunky_adaptive_params;
/* Fills the defaults: threshold 0.05, floor 0.01, min_spp 16, check_interval 16.  The threshold is a PLACEHOLDER that has not been
 * tuned on the device yet (DESIGN.md section 13 says what is missing): set it yourself until it is. */
int chunky_adaptive_default_params(chunky_adaptive_params* p);

/* What one chunky_render_adaptive call did.  active[i] = active pixels after the i-th check, for the first
 * CHUNKY_ADAPTIVE_MAX_CHECKS checks; `checks` counts all of them (it may exceed the array). */
#define CHUNKY_ADAPTIVE_MAX_CHECKS 64
typedef struct chunky_adaptive_summary {
    int32_t rounds;   /* rounds of passes rendered (the first of min_spp passes, the others of check_interval or what was left) */
    int32_t checks;   /* checks run */
    int32_t passes;   /* passes rendered on the pixels that stayed to the end (<= max_spp) */
    int32_t reserved;
    int64_t samples;  /* samples rendered: the sum of count[p] over the image */
    int32_t active[CHUNKY_ADAPTIVE_MAX_CHECKS];
} chunky_adaptive_summary;

/* The specification as code: needs no context and no device.  samples = n images [n][height][width][3], the sample of pass k of every
 * pixel; n is max_spp.  count_out: width * height; mean_out: 3 * width * height, the running mean at each pixel's n_p; stat_out:
 * 2 * width * height, (m, M2) per pixel.  Any output may be NULL.  CHUNKY_E_INVALID for: a params.size smaller than the first version
 * of the struct, a threshold that is not finite or < 0, a floor that is not finite and > 0, min_spp < 2, check_interval < 1, unknown
 * flag bits, n < min_spp. */
int chunky_adaptive_host(int width, int height, const float* samples, int n, const chunky_adaptive_params* params,
                         int32_t* count_out, float* mean_out, float* stat_out);

/* Renders adaptively, blocking: resets the framebuffer and the adaptive state, then runs rounds — min_spp passes, then check_interval
 * at a time, pass k with seeds[k] — each followed by a check, until no pixel is active or max_spp passes are done.  While every pixel
 * is active a round is an ordinary launch; afterwards the active pixels are rendered from a list built on the device in the order of
 * the kernel's pixel slots (the same list on every run).  summary_out may be NULL.  Afterwards chunky_render_read,
 * chunky_render_denoise and the AOV calls see the adaptive image like any other; the target's shard and options are untouched.
 * Parameter errors as chunky_adaptive_host (max_spp in the place of n).  CHUNKY_E_STATE, never a fallback: a group's target, a target
 * with a shard of world > 1, and a scene / option set that the staged-sample kernel (render_pool) does not take — the statistic is
 * computed from the staged samples, which only that kernel writes. */
int chunky_render_adaptive(chunky_render* r, const int32_t* seeds, int max_spp, const chunky_adaptive_params* params,
                           chunky_adaptive_summary* summary_out);
/* The maps of the last adaptive run: count[p] (n must be width * height) and (m, M2)[p] (n_floats must be 2 * width * height).
 * CHUNKY_E_STATE before any adaptive run on the target. */
int chunky_render_adaptive_counts(chunky_render* r, int32_t* out, int64_t n);
int chunky_render_adaptive_noise(chunky_render* r, float* out, int64_t n_floats);
/* Device time of the adaptive runs since the last call — their render launches, folds, checks and compactions — and the number of
 * rounds; apart from chunky_render_kernel_time, which does not see them.  A check that chunky_render_adaptive_resume makes before its
 * first round (the one the earlier run left out) is in total_ms and counts as no round; chunky_render_adaptive_restore is not timed. */
int chunky_render_adaptive_kernel_time(chunky_render* r, float* total_ms, int* rounds);
/* ---- self test of the list route: renders n passes (seeds[k], bufferSpp k) on the listed pixels only, through the launch the later
 * rounds of chunky_render_adaptive use (the staged-sample kernel over a device-resident list of pixel indices), folding into the
 * framebuffer as it is.  pixels: n_pixels distinct indices y * width + x in any order.  Blocking.  Same state errors as
 * chunky_render_adaptive. */
int chunky_selftest_render_list(chunky_render* r, const int32_t* pixels, int n_pixels, const int32_t* seeds, int n);
/* ---- self test of the biome-tint launch plan (host only, needs no device): for n launch plans of 16 ints each — family (0 the pool
 * kernel, 1 render_waves, 2 render_lanes), tree form, parked paths, words, lanes per pixel, stack entries, entity BVHs, extended
 * integrator, statistics, sorted block tests, projected camera, LDS bytes, most passes, needs the pixel list, status (0 ok), the
 * extended options' refusal — out16 receives the plan of the kernels that tint by position in the same layout and refusal[i] why
 * there is none (0: there is one; 1 phase statistics, 2 the extended options, 3 a projected camera on the pool kernel). */
int chunky_selftest_plan_biome(const int32_t* plans16, int64_t n, int32_t* out16, int32_t* refusal);

/* ---- adaptive sampling that stops and continues: pause, a raised SPP target, a render dump reloaded after a restart ----
 * A run is described by its state after `passes` passes; every active pixel has seen exactly those passes.  Beside this header the
 * state has four arrays: mean (3 * W * H floats, the image), count (W * H ints), stat (2 * W * H floats, (m, M2)) and active (W * H
 * bytes, each 0 or 1).  The map cannot be derived from the rest: a pixel that left at a check at `passes` and a pixel that is still
 * active both have count == passes.
 *
 * The check points are the grid min_spp + j * check_interval (j >= 0).  Continuing a state to max_spp > passes (adaptive_spec.h
 * ad_step): first, when a check at `passes` is due under the new max_spp (passes on the grid, passes < max_spp) and last_check !=
 * passes, that check is run — the earlier run ended there on its own max_spp, where none is made.  Then rounds up to the next grid
 * point or to max_spp, whichever comes first (a state off the grid — stopped inside a round, or ended on an off-grid max_spp — takes a
 * short round first), each followed by its check when one is due.  chunky_render_adaptive is this loop from the empty state.
 *
 * Two properties, both bit for bit in image, counts and (m, M2):
 *   P1  stop = shorter run: for d >= min_spp the state after d passes is the result of chunky_adaptive_host(samples[0 .. d), n = d),
 *       whether or not the check at d has been run (who leaves at d and who stays both record d).
 *   P2  resume = fresh: the start state continued over any split 0 < d1 < ... < B of the passes equals chunky_adaptive_host(samples, B);
 *       summary.checks, .active[], .samples and .passes equal the single run's (.rounds may differ: a split can cut a round in two). */
typedef struct chunky_adaptive_state {
    size_t size;          /* sizeof(chunky_adaptive_state) as the caller was compiled; members may be appended */
    int32_t width, height;
    int32_t passes;       /* passes folded into every still-active pixel */
    int32_t last_check;   /* pass count at which the last check ran, 0 = none yet */
    int32_t active;       /* number of active pixels */
    int32_t reserved;
    chunky_adaptive_params params;
    chunky_adaptive_summary summary; /* cumulative from pass 0 */
} chunky_adaptive_state;

/* The host side of it: no context and no device.  _begin writes the start state (passes 0, every pixel active, everything else 0;
 * params as chunky_adaptive_host takes them, without the n >= min_spp rule) into st and the four arrays.  _resume continues st and the
 * arrays in place with `samples`, n images [n][height][width][3]: the samples of passes st->passes .. st->passes + n - 1; the target is
 * max_spp = st->passes + n.  n may be smaller than min_spp (nothing is checked before min_spp; every count is then the pass count); n
 * == 0, or a state with no active pixel, changes nothing.  _resume validates the state with chunky_adaptive_state_check first. */
int chunky_adaptive_host_begin(int width, int height, const chunky_adaptive_params* params, chunky_adaptive_state* st, int32_t* count,
                               float* mean, float* stat, uint8_t* active);
int chunky_adaptive_host_resume(chunky_adaptive_state* st, const float* samples, int n, int32_t* count, float* mean, float* stat,
                                uint8_t* active);
/* CHUNKY_OK for a state a run can have left, CHUNKY_E_INVALID (with the rule in the message) otherwise: size at least this struct's;
 * width, height > 0 and small enough for chunky_adaptive_host; params valid by its rules; passes >= 0; last_check is 0 when no grid
 * point is <= passes, else the largest grid point g <= passes or — only when g == passes — the grid point before it (0 if none);
 * active[p] is 0 or 1; an active pixel has count == passes; an inactive pixel's count is on the grid and <= last_check; st->active is
 * the number of ones in the map; summary.passes == passes; summary.samples == the sum of count.  mean and stat are not inspected
 * (non-finite values are legal there: see the convergence test above). */
int chunky_adaptive_state_check(const chunky_adaptive_state* st, const int32_t* count, const uint8_t* active);

/* Hooks of an adaptive run (any pointer may be NULL; struct_size as chunky_run_callbacks::struct_size):
 *   post_render  polled before every render launch (a round longer than the launch cap is several launches) and after every round's
 *                check; non-zero ends the call with CHUNKY_E_ABORTED.  The target is then at a launch boundary: the pixels still
 *                active have recorded the passes done, image, counts and noise are readable and equal P1 for those passes, and the
 *                state continues with chunky_render_adaptive_resume.
 *   round_done   after every round (and its check): the pass count and the number of active pixels.
 * Both run with the context locked: they must not call into the library on that context (another thread that does waits for the run). */
typedef struct chunky_adaptive_callbacks {
    size_t struct_size;
    int (*post_render)(void* user);
    void (*round_done)(void* user, int32_t passes, int32_t active);
    void* user;
} chunky_adaptive_callbacks;

/* chunky_render_adaptive with the hooks: from pass 0, resetting the framebuffer and the adaptive state.  chunky_render_adaptive is
 * this call with callbacks == NULL.  summary_out receives the summary so far on CHUNKY_OK and on CHUNKY_E_ABORTED. */
int chunky_render_adaptive_ex(chunky_render* r, const int32_t* seeds, int max_spp, const chunky_adaptive_params* params,
                              const chunky_adaptive_callbacks* callbacks, chunky_adaptive_summary* summary_out);
/* Continues from the state the target holds — left by chunky_render_adaptive, _ex or _resume (finished or aborted) or by _restore —
 * to max_spp passes, pass k with seeds[k]: `seeds` is the SAME stream from pass 0 (max_spp values; a contract, not checked), of
 * which seeds[passes ..) are used.  The result obeys P2; the summary is cumulative from pass 0.  params must equal the state's
 * (threshold, floor, min_spp, check_interval), else CHUNKY_E_STATE: continuing under other parameters is not supported (an inactive
 * pixel never becomes active again).  max_spp == passes, or no active pixel: CHUNKY_OK, nothing rendered.  max_spp < passes:
 * CHUNKY_E_INVALID.  CHUNKY_E_STATE when the target holds no state to continue: none was ever left, or a call that writes the
 * framebuffer or changes what a pass renders came since (one that was refused with an error before it changed anything ends nothing) — chunky_render_passes, chunky_render_run / _run_ex, chunky_render_reset,
 * chunky_selftest_render_list, chunky_render_set_device_buffer, _set_camera, _set_option, _set_shard.  The AOV and denoise calls do
 * not end it (chunky_render_adaptive_counts / _noise stay readable through all of these, as before).  Scene uploads between the two
 * calls are the caller's contract, as they are between two chunky_render_passes calls: the passes to come render the scene as it is
 * then.  Other state errors as chunky_render_adaptive. */
int chunky_render_adaptive_resume(chunky_render* r, const int32_t* seeds, int max_spp, const chunky_adaptive_params* params,
                                  const chunky_adaptive_callbacks* callbacks, chunky_adaptive_summary* summary_out);
/* The header of the target's state and its activity map (n must be width * height; active_out may be NULL); image, counts and noise
 * come from chunky_render_read, chunky_render_adaptive_counts and _noise.  CHUNKY_E_STATE as chunky_render_adaptive_resume. */
int chunky_render_adaptive_state(chunky_render* r, chunky_adaptive_state* out, uint8_t* active_out, int64_t n);
/* Takes a state onto a target of the same width and height that chunky_render_adaptive accepts (no group, no shard of world > 1, a
 * scene and options render_pool takes): validates it with chunky_adaptive_state_check, uploads mean into the framebuffer (the
 * caller-owned device buffer when one is set), count, stat and the map, and rebuilds the active list on the device in the order the
 * original run held it.  The target then continues with chunky_render_adaptive_resume.  CHUNKY_E_INVALID (a NULL array, a size
 * mismatch, an invalid state) and CHUNKY_E_STATE leave the target as it was. */
int chunky_render_adaptive_restore(chunky_render* r, const chunky_adaptive_state* st, const float* mean, const int32_t* count,
                                   const float* stat, const uint8_t* active);

/* ---- firefly-robust accumulation: bucket means and a Gini-trimmed resolve ----
 * No counterpart in the reference (its image is the plain running mean, in which one sample thousands of times brighter than its
 * neighbours stays visible for thousands of passes).  The method is a median of means with an adaptive trim, after the idea of
 * Buisine, Delepoulle and Renaud, "Firefly removal in Monte Carlo rendering with adaptive Median of meaNs" (2021); the formulas are
 * this project's own specification and do not claim to reproduce that paper.  The arithmetic is chunkyclplugin_amd/csrc/robust_spec.h,
 * compiled by the kernels and the host alike; every operation is ONE exactly rounded float operation, no multiply-add is fused.
 *
 * Buckets.  M is odd, 3 <= M <= 15, h = (M - 1) / 2.  The target counts robust samples from 0 since chunky_render_robust_begin; sample
 * j goes to bucket j % M, whose mean is updated per channel as the framebuffer's is (K/rayTracer.cl:109-112) with k = j / M:
 *     mean_b = (mean_b * (float)k + c) / (float)(k + 1)
 * first_buffer_spp weights only the beauty mean (the framebuffer), exactly as in chunky_render_passes.
 *
 * Resolve, per pixel and per channel, over the M bucket means x:
 *   1. sort ascending with the fixed odd-even transposition network: rounds r = 0 .. M - 1, round r compares the pairs (i, i + 1) for
 *      i = r & 1, (r & 1) + 2, ... and swaps iff x[i + 1] < x[i].  A NaN never swaps; the order is then defined but arbitrary.
 *   2. S = x0; S = S + x_i for i = 1 .. M - 1.   W = (float)(1 - M) * x0; W = W + (float)(2 i - M + 1) * x_i for i = 1 .. M - 1.
 *   3. G = (S > 0 && S < inf) ? W / ((float)M * S) : 0 (the Gini coefficient of the bucket means; a NaN in S gives 0).
 *   4. p = (G * (float)(h + 1)) * gain;  t = !(p > 0) ? 0 : (p >= (float)h ? h : (int)p).  CHUNKY_ROBUST_MEAN forces t = 0,
 *      CHUNKY_ROBUST_MEDIAN forces t = h, CHUNKY_ROBUST_GINI uses the formula.
 *   5. out = (x_t + x_{t+1} + ... + x_{M-1-t}) / (float)(M - 2 t), added left to right.
 * The trim byte of a pixel is the largest t of its three channels.
 *
 * The resolved image is a BIASED estimator: it darkens legitimately rare bright paths (a small light seen through a long diffuse
 * chain) as it darkens fireflies.  It is not the reference's image.  The beauty image — chunky_render_read — is unchanged by all of
 * this: chunky_render_robust_passes folds it bit for bit as chunky_render_passes does. */
#define CHUNKY_ROBUST_MEAN 0
#define CHUNKY_ROBUST_MEDIAN 1
#define CHUNKY_ROBUST_GINI 2
#define CHUNKY_ROBUST_MIN_BUCKETS 3
#define CHUNKY_ROBUST_MAX_BUCKETS 15
typedef struct chunky_robust_params {
    int32_t size; /* sizeof(chunky_robust_params) as the caller was compiled (members may be appended) */
    int32_t mode; /* CHUNKY_ROBUST_MEAN, _MEDIAN or _GINI */
    float gain;   /* finite, >= 0: scales the trim of CHUNKY_ROBUST_GINI (0 trims nothing); checked in every mode */
} chunky_robust_params;
/* Fills the defaults: CHUNKY_ROBUST_GINI with gain 1. */
int chunky_robust_default_params(chunky_robust_params* p);

/* The bucket fold on the host: needs no context and no device.  samples = n images [n][height][width][3], the robust samples
 * first_index .. first_index + n - 1 of every pixel; buckets = n_buckets images [bucket][height][width][3], the state before (all
 * zero at the start) and after.  n == 0 is legal.  CHUNKY_E_INVALID: a NULL array, width or height <= 0, an even n_buckets or one
 * outside 3 .. 15, n < 0, first_index < 0 or first_index + n beyond INT32_MAX. */
int chunky_robust_host(int width, int height, const float* samples, int n, int n_buckets, int first_index, float* buckets);
/* The resolve on the host, the specification the device is held to: buckets [n_buckets][n_pixels][3] to out (3 * n_pixels floats)
 * and, where trim is not NULL, the trim bytes (n_pixels).  Whether a bucket holds a sample is the caller's affair here.
 * CHUNKY_E_INVALID: a NULL array, n_pixels <= 0, a bad n_buckets, params NULL or with a size below this struct's first version
 * (through `gain`), an unknown mode, a gain that is not finite or < 0. */
int chunky_robust_host_resolve(int n_buckets, int64_t n_pixels, const float* buckets, const chunky_robust_params* params, float* out,
                               uint8_t* trim);

/* Allocates and zeroes the target's n_buckets bucket images, laid out [bucket][pixel][3], and sets the robust sample count to 0; a
 * second call resets the state (to another n_buckets where asked); n_buckets == 0 releases it.  Waits for the target's queued work.
 * The framebuffer is not touched.  CHUNKY_E_INVALID for an even n_buckets or one outside 3 .. 15; CHUNKY_E_STATE for a group's
 * target.  No other call sees or touches the robust state (chunky_render_reset included), and the robust calls touch no other
 * image than the framebuffer, which chunky_render_robust_passes folds as chunky_render_passes does. */
int chunky_render_robust_begin(chunky_render* r, int n_buckets);
/* chunky_render_passes plus the bucket fold: n passes (seeds[k], bufferSpp first_buffer_spp + k) folded into the framebuffer bit
 * for bit as chunky_render_passes folds them, and as robust samples count .. count + n - 1 into the buckets, from one read of the
 * staged samples.  Asynchronous, in launches of at most 256 passes (fewer where the staging array would pass its cap); n == 0 is
 * legal.  A chunky_render_passes between two of these calls adds to the framebuffer only.  A shard set with chunky_render_set_shard
 * is honoured: a rank folds its own pixels and leaves the others' buckets zero.
 * CHUNKY_E_INVALID: n < 0, NULL seeds with n > 0, first_buffer_spp < 0, a count that would pass INT32_MAX.  CHUNKY_E_STATE, never a
 * fallback and before anything is launched: before chunky_render_robust_begin or chunky_render_set_camera; a group's target; a scene
 * or options that send the target to the fallback kernels, which stage no samples; a biome map on the scene while the target tints
 * by position; the extended light-transport options where chunky_render_passes refuses them. */
int chunky_render_robust_passes(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp);
/* Blocking read-back of bucket b (0 .. n_buckets - 1), 3 * width * height floats; *count (may be NULL) receives the robust sample
 * count.  CHUNKY_E_STATE before chunky_render_robust_begin; CHUNKY_E_INVALID for a bucket outside the range, a NULL buffer or a
 * wrong n_floats. */
int chunky_render_robust_read_bucket(chunky_render* r, int b, float* out, int64_t n_floats, int32_t* count);
/* The resolve on the device, blocking: out receives the image (n_floats = 3 * width * height) and trim, where not NULL, the trim
 * bytes (n_pixels = width * height; ignored with trim == NULL).  The buckets and the framebuffer are read, never written.
 * Parameter errors as chunky_robust_host_resolve.  CHUNKY_E_STATE before chunky_render_robust_begin, and while fewer than n_buckets
 * samples have been folded (a bucket would be empty). */
int chunky_render_robust_resolve(chunky_render* r, const chunky_robust_params* params, float* out, int64_t n_floats, uint8_t* trim,
                                 int64_t n_pixels);
/* chunky_render_denoise with the resolved image in the place of the framebuffer: resolved and filtered on the device with the
 * target's own AOV images, only the result crosses to the host.  Errors as chunky_render_robust_resolve and chunky_render_denoise
 * (CHUNKY_E_STATE before any AOV pass and on a shard of world > 1); its launches are timed with the denoiser's
 * (chunky_render_denoise_kernel_time). */
int chunky_render_robust_denoise(chunky_render* r, const chunky_robust_params* robust_params, const chunky_denoise_params* denoise_params,
                                 float* out, int64_t n_floats);
/* Device time of the chunky_render_robust_passes launches (render kernel and fold) and of the resolve kernels since the last call,
 * from HIP events on the stream they run on, and the number of render launches; apart from chunky_render_kernel_time, which does
 * not see them.  resolve_ms (may be NULL, as the others) receives the resolves' share on its own; it is not in total_ms. */
int chunky_render_robust_kernel_time(chunky_render* r, float* total_ms, int* launches, float* resolve_ms);
/* ---- self test of the two robust kernels on caller-supplied samples (how non-finite values reach the device): samples = n images
 * [n][height][width][3] are arranged on the device in the staging layout of one launch of the whole image, folded from zero buckets
 * as robust samples first_index .. by the fold kernel, and resolved.  buckets_out (3 * n_buckets * width * height floats), image_out
 * (3 * width * height) and trim_out (width * height bytes) may each be NULL.  1 <= n <= 256, width * height <= 2^20; parameter errors
 * as chunky_robust_host and chunky_robust_host_resolve.  Blocking. */
int chunky_selftest_robust(chunky_ctx* ctx, int width, int height, const float* samples, int n, int n_buckets, int first_index,
                           const chunky_robust_params* params, float* buckets_out, float* image_out, uint8_t* trim_out);

/* ---- host pass loop (replaces OpenClPathTracingRenderer.render, J/opencl/OpenClPathTracingRenderer.java:54-191):
 * seeds from java.util.Random(0).nextInt(), bufferSpp restarting at 0 after each read-back, merge
 * sample = (sample*sampSpp + pass*passSpp) / (sampSpp+passSpp) in double (:167-173).
 * `sample_buffer` is Chunky's double[3*W*H]; `*scene_spp` its scene.spp (in/out).  `post_render`
 * (may be NULL) is polled at least every 100 ms and at every merge; non-zero stops the loop
 * (:153-157,163).  `merge_interval` = passes per read-back (the reference uses 1024, :158). */
typedef int (*chunky_post_render_fn)(void* user);
int chunky_render_run(chunky_render* r, double* sample_buffer, int32_t* scene_spp, int32_t target_spp,
                      int32_t merge_interval, chunky_post_render_fn post_render, void* user);

/* The same loop with every hook the reference's loop has (any pointer may be NULL):
 *   post_render       BooleanSupplier postRender: polled at least every 100 ms between launches and before every merge;
 *                     non-zero stops the loop (OpenClPathTracingRenderer.java:153-157,163,181).
 *   progress          after every launch, with the new scene.spp (the reference increments scene.spp per pass, :144).
 *   merged            after every merge into sample_buffer, with the spp the sample buffer now holds: the place of
 *                     scene.postProcessFrame + manager.redrawScreen (:172-177).  sample_buffer is complete and not
 *                     touched by the library while the callback runs.
 *   save_event        the two conditions that force a merge (:150): returns 1 when isSaveEvent(manager.getSnapshotControl(),
 *                     scene, spp) holds (:193-195) — a snapshot or render dump is due when the scene reaches `spp` — and 2 when
 *                     only scene.shouldFinalizeBuffer() does.  The loop asks for every spp the next launch would cover and cuts
 *                     the launch there, merges at once (:151,162-178); after a 1 it polls post_render once more after `merged`
 *                     (the reference makes that poll for real save events only, :179-182), after a 2 it does not.
 *   poll_gate         consulted before the TIMED poll only (the reference's `!manager.shouldFinalize()`, :154): zero skips that
 *                     poll.  The polls before a merge (:163) and after a save event (:181) are unconditional, as in the reference.
 *   regenerate_camera between launches, for projections other than pinhole: the reference re-generates the jittered
 *                     camera-ray table on a worker while passes run (:146-148, ClCamera.java:72-104).  The hook may
 *                     call chunky_render_set_camera (from this or any other thread: the context mutex is the
 *                     reference's renderLock) to install a fresh table; passes already queued finish with the old one.
 * chunky_render_run(..., post_render, user) is chunky_render_run_ex with only post_render set.
 * struct_size = sizeof(chunky_run_callbacks) as the CALLER was compiled: members are appended over time, and the library reads
 * only those the caller's struct holds (a host built against an older header keeps working; 0 or a size that cuts a member in
 * half is CHUNKY_E_INVALID). */
typedef struct chunky_run_callbacks {
    size_t struct_size;
    int (*post_render)(void* user);
    void (*progress)(void* user, int32_t scene_spp);
    void (*merged)(void* user, int32_t sample_spp);
    int (*save_event)(void* user, int32_t spp);
    void (*regenerate_camera)(void* user);
    void* user;
    int (*poll_gate)(void* user);
} chunky_run_callbacks;
int chunky_render_run_ex(chunky_render* r, double* sample_buffer, int32_t* scene_spp, int32_t target_spp,
                         int32_t merge_interval, const chunky_run_callbacks* callbacks);
/* The seed stream itself: first n values of new java.util.Random(seed).nextInt(). */
int chunky_java_random_ints(int64_t seed, int32_t* out, int n);

/* ---- tone mapping: the `filter` kernel (tonemap/include/post_processing_filter.cl:5-51) ----------------
 * Replaces GpuPostProcessingFilter.processFrame (GpuPostProcessingFilter.java:40-65): `input` is Chunky's
 * sample buffer, 3 doubles (R, G, B) per pixel; `argb_out` receives width*height words 0xFFRRGGBB.  `exposure`
 * is narrowed to float as the reference does (:53).  type: 0 GAMMA, 1 TONEMAP1, 2 ACES ("TONEMAP2"), 3 HABLE
 * ("TONEMAP3") (ImposterCombinationGpuPostProcessingFilter.java:11-15); any other value applies the exposure
 * only, like the reference's switch without a default.  Blocking; copies in and out (CL_MEM_COPY_HOST_PTR +
 * blocking read in the reference). */
#define CHUNKY_FILTER_GAMMA 0
#define CHUNKY_FILTER_TONEMAP1 1
#define CHUNKY_FILTER_ACES 2
#define CHUNKY_FILTER_HABLE 3
int chunky_filter_frame(chunky_ctx* ctx, int width, int height, double exposure, const double* input,
                        int32_t* argb_out, int type);
/* The same tone map with the alpha byte of pixel p taken from alpha[p] (width*height floats, e.g. the CHUNKY_AOV_ALPHA image:
 * Chunky's "transparent sky") instead of 0xFF: the byte is min(255, (uint)(clamp(alpha, 0, 1) * 255.0f + 0.5f)), 0 for a NaN.
 * R, G and B are byte-identical to chunky_filter_frame's. */
int chunky_filter_frame_alpha(chunky_ctx* ctx, int width, int height, double exposure, const double* input, const float* alpha,
                              int32_t* argb_out, int type);
/* Host-side instrument (no device needed): that alpha byte for each of n values, from the function the kernel compiles. */
int chunky_filter_alpha_bytes(const float* alpha, int64_t n, int32_t* out);
/* Host-side instrument (no device needed): the 256 thresholds the GAMMA / ACES curves are evaluated with — T[k] = the smallest
 * float c >= 0 whose output byte min(255, (uint)(pow(c, 1/2.2) * 255 + 0.5)) is >= k (post_processing_filter.cl:24-27,
 * rgba.h:9-14).  The byte is a monotone step function of c, so comparing c with these is the same function as evaluating
 * pow; tests/test_filter.py checks that over every float. */
int chunky_filter_gamma_thresholds(float* out256);
/* Same kernel on buffers already in device memory (`d_input`: 3*n_pixels doubles, `d_argb`: n_pixels words),
 * enqueued `repeat` times on the context's stream and waited for; *kernel_ms (may be NULL) receives the mean
 * device time of one launch from HIP events on that stream. */
int chunky_filter_frame_device(chunky_ctx* ctx, int64_t n_pixels, float exposure, const void* d_input, void* d_argb,
                               int type, int repeat, float* kernel_ms);

/* ---- host-side verification hook for the octree re-layout done at upload (no device needed):
 * builds the wide tree of chunkyclplugin_amd/csrc/widetree.hpp from `tree` and looks n cells up in
 * it, returning for each the block pointer (K/octree.h:88) and the leaf level.  level_bits == NULL
 * uses the default split.  *n_entries receives the size of the re-laid-out array. */
int chunky_widetree_lookup(const int32_t* tree, int64_t n_ints, int depth, const int32_t* level_bits, int n_levels,
                           const int32_t* xyz /* 3n */, int n, int32_t* data_out, int32_t* level_out, int64_t* n_entries);
/* The same tree annotated with the block palette `blocks` (as the upload does): *hit_top = 1 + the highest cell y of any leaf that
 * can be hit — 0 when none can, 2^depth when one reaches the world's top.  render_pool ends the march of a ray that runs upwards
 * once it is at or above that height. */
int chunky_widetree_hit_top(const int32_t* tree, int64_t n_ints, int depth, const int32_t* level_bits, int n_levels,
                            const int32_t* blocks, int64_t n_block_ints, int32_t* hit_top);
/* The hit_top the next launch on this scene carries (needs a complete scene, as a launch does; 2^depth for a scene whose octree has
 * no wide tree).  On a group: member 0's. */
int chunky_scene_hit_top(chunky_scene* scene, int32_t* hit_top);

/* ---- host-side verification hook for how the kernels address scene arrays (no device needed).  At upload the library decides, per
 * array, whether kernels may read it as "base + 32-bit unsigned byte offset" (DESIGN.md section 5).  chunky_addr32_word is that
 * decision: dims = {atlas width, height, layers, sky width, height}, bytes = the sizes in bytes of the model-record arrays {aabb_rec,
 * quad_rec}, indices_checked = those arrays are the library's own, built from the palettes as they are.  *word: bit 0 the
 * atlas, bit 1 the sky, bit 2 the record arrays.  A scene whose word lacks a bit renders on kernels with 64-bit addresses. */
int chunky_addr32_word(const int64_t dims[5], const uint64_t bytes[2], int indices_checked, uint32_t* word);
/* The word the next launch on this scene carries (needs a complete scene, as a launch does).  On a group: member 0's. */
int chunky_scene_addr32(chunky_scene* scene, uint32_t* word);

/* ---- self test: evaluate the rt_math.h contract on the device (bit-compared with the host by tests) */
int chunky_selftest_math(chunky_ctx* ctx, int which, int n, const float* a, const float* b, float* out);

/* ---- self test: helper-level known answers (no reference counterpart as an entry point).
 * Evaluates, one call per input row, the device functions the kernels are made of — the counterparts of the reference's
 * helpers K/primitives.h:30-162 (AABB_quick_intersect 0, AABB_exit 1, AABB_full_intersect 2, AABB_full_intersect_map_2 3),
 * K/block.h:30-118 (BlockPalette_intersectBlock 4: cube, AABB-model and quad-model blocks with their materials),
 * K/primitives.h:335-409 (Triangle_new + Triangle_intersect 6), K/sky.h:42-106 (Sun_sampleDirection 7, Sun_intersect 8,
 * Sky_intersect 9), K/kernel.h:46-98 (nextPath 10), K/textureAtlas.h:18-28 (Atlas_read_uv 11), K/material.h:31-82
 * (Material_get + Material_sample 12), K/octree.h:41-109 (Octree_octreeIntersect 14; `tree` 0 = the reference layout, 1 = the
 * wide tree in the form the render kernels pick, reported in *tree_used), K/bvh.h:22-113 (Bvh_intersect on the world BVH: 15
 * on the packed arrays, 18 as the pool kernel walks its aligned records) — on the scene's own palettes, atlas, sky and sun.
 * Rows are 32 floats in and 12 out (ints as their bit patterns); the layouts are listed in oracle/ref_shim.cpp ref_helpers,
 * which produced tests/golden/helpers.npz from the reference object itself.  A parity failure then names a function, not a pixel. */
int chunky_selftest_helpers(chunky_scene* scene, int which, int tree, int n, const float* in_rows, float* out_rows, int32_t* tree_used);

/* ---- self test of the projected camera: the device function the render kernels use, run over all width*height pixels of the
 * target's camera for `seed`, with its lens if one is set; out receives width*height*6 floats (n_floats must be that), as
 * chunky_camera_rays(_lens) lays them out.  CHUNKY_E_STATE unless the target has a projected camera. */
int chunky_selftest_camera_rays(chunky_render* r, int32_t seed, float* out, int64_t n_floats);

/* ---- self test of the shard-to-pixel map (no reference counterpart): the device functions every image-writing kernel takes its
 * pixels from, on the view chunky_render_set_shard would store for (rank, world, tile) on a width x height image (view_out, if not
 * NULL, receives it: rank, world, the clamped tile, the rank's pixel slots n_local).  mode 0: for slots 0 .. n - 1 — slots at and
 * beyond n_local are part of the domain — out receives 5 ints per slot: the slot's pixel index (width * height for a padding
 * slot), the pixel index / column / row as the pool kernel derives them for a new sample, and the run formula's pixel index where
 * it applies (one rank or tile > 0, slot < n_local; -1 elsewhere).  mode 1: `pairs` holds n pairs (a, d) of uint32 with
 * a < 2^31, d >= 1; out receives the n quotients a / d as the kernels compute them (one multiply-high and one shift by a pair
 * made on the host); width .. tile are ignored.  n <= 2^24. */
int chunky_selftest_shard_map(chunky_ctx* ctx, int mode, int width, int height, int rank, int world, int tile, int n,
                              const uint32_t* pairs, int32_t* out, int32_t view_out[4]);

/* ---- self test of the tone map's byte estimate (no reference counterpart): `count` consecutive float bit patterns from
 * first_bits through the fast path of the GAMMA (curve 0) or ACES (curve 2) filter (hardware log2 / exp2 / reciprocal
 * estimate, settled against the threshold table — ACES: after the correctly rounded division — only near a step) and
 * through the reference's arithmetic (post_processing_filter.cl:33-38 for ACES) followed by a plain search of
 * chunky_filter_gamma_thresholds' table; *mismatches = values whose bytes differ (must be 0), *worst_estimate = the
 * furthest an estimate strayed beyond its byte's interval (may be NULL). */
int chunky_selftest_gamma_scan(chunky_ctx* ctx, int curve, uint32_t first_bits, uint64_t count, uint64_t* mismatches, float* worst_estimate);

#ifdef __cplusplus
}
#endif
#endif /* CHUNKY_HIP_H */
