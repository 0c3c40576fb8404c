/*
 * nmf.h — C ABI of the MI355X-native batched NeuroMechFly stepping engine (libnmf_hip.so).
 *
 * The reference has no FFI for this path: its "operator API" is the Python class
 * flygym.warp.GPUSimulation (reference src/flygym/warp/simulation.py:28-453), which forwards
 * to mujoco_warp.  Each entry point below replaces one group of those calls; the Python class
 * flygym_amd.HIPSimulation binds them with ctypes (see INTEGRATION.md for the stub a flygym
 * maintainer would add).  No torch / HIP types appear in the signatures: device buffers are
 * plain pointers, streams are passed as void* (hipStream_t), sizes are ints.
 *
 * All device arrays are float32, row-major, world-major: field[n_worlds][width].
 * All calls are stream-ordered device work without host synchronisation (hipGraph-capturable)
 * unless stated otherwise.  Return value: 0 on success, negative on error (see nmf_last_error).
 */
#ifndef NMF_H_
#define NMF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nmf_model nmf_model;
typedef struct nmf_batch nmf_batch;
typedef struct nmf_eye_plan nmf_eye_plan;
typedef struct nmf_camera_plan nmf_camera_plan;
typedef struct nmf_cpg nmf_cpg;
typedef struct nmf_plume nmf_plume;
typedef struct nmf_odometry nmf_odometry;
typedef struct nmf_motion nmf_motion;
typedef struct nmf_navigator nmf_navigator;
typedef struct nmf_stabilizer nmf_stabilizer;
typedef struct nmf_rules nmf_rules;
typedef struct nmf_visnet nmf_visnet;
typedef struct nmf_task nmf_task;

/* Per-world fields addressable through nmf_field_ptr / nmf_gather_* */
enum nmf_field {
  NMF_QPOS = 0,         /* [nq]      generalized positions (free joint 7 + hinges)            */
  NMF_QVEL = 1,         /* [nv]                                                                */
  NMF_CTRL = 2,         /* [nu]      actuator controls                                         */
  NMF_QACC_WARMSTART = 3, /* [nv]                                                              */
  NMF_SEG_XPOS = 4,     /* [nseg*3]  world positions of the named body segments               */
  NMF_SEG_XQUAT = 5,    /* [nseg*4]  world orientations (w,x,y,z)                              */
  NMF_SITE_XPOS = 6,    /* [nsite*3]                                                           */
  NMF_ACTUATOR_FORCE = 7, /* [nu]                                                              */
  NMF_SENSORDATA = 8,   /* [96]      6 legs x (found, force3, torque3, pos3, normal3, tangent3)*/
  NMF_TIME = 9,         /* [1]                                                                 */
  NMF_STATS = 10,       /* [8]       of the launch's last step, as floats: ncon, solver iterations, overflow flag, nefc, solve-report
                                    bits (bit k = column 4 + k of NMF_STATS_SUM), most pivots of an elimination, KKT residual of
                                    the last elimination's target (0 = exact end; contact-space solve only), 0                */
  NMF_QACC = 11,        /* [nv]                                                                */
  NMF_COST = 12,        /* [1]       shader cycles the world took in the last stepping launch (load metric) */
  NMF_STATS_SUM = 13,   /* [16]      since the last reset, uint32_t COUNTERS (read them through a uint32_t / int32_t view of the
                                    pointer nmf_field_ptr returns; means over any window = differences of two reads; exact up to
                                    4.29e9, i.e. ~7e8 steps of one world at 6 contacts per step between two resets):
                                    0 physics steps, 1 sum of ncon, 2 sum of solver iterations, 3 steps with contact overflow;
                                    how the steps' constraint solves ended — 4 solved in contact space, of which 5 exactly (the
                                    elimination's target satisfies its own active set: KKT), 6 by the tie rule, 7 after a fourth
                                    line search without measurable descent, 8 by the cost tests, 9 at the iteration limit;
                                    10 solved by the primal Newton loop, of which 11 after a contact-space solve whose end failed
                                    the residual test; 12 steps with an elimination of more than 47 pivots; 13 steps with contacts
                                    that could not take the CPU flavour's noslip pass; 14 steps without contact; 15 unused    */
  NMF_CONTACT_GEOM = 14, /* [48]     contact list of the launch's last step: index (into the world's contact-geom list,
                                    reference compose/world.py:300-309 pair order sorted by body) of the geom of contact
                                    c, as a float; -1 beyond ncon                                                    */
  NMF_ACT = 15,         /* [nu]      activation state of the stateful actuators (intvelocity, cylinder, muscle: MuJoCo's act, here one
                                    slot per actuator — 0 for the stateless ones); reset to 0; writable between launches       */
  NMF_FIELD_COUNT = 16
};

/* Text of the last error raised on the calling thread ("" if none). */
const char* nmf_last_error(void);

/* Parse a compiled-model blob (flygym_amd.compiler.model.CompiledModel.to_blob()).
 * Replaces: world.compile() + mjw.put_model  (reference simulation.py:37, warp/simulation.py:417). */
nmf_model* nmf_model_create(const void* blob, size_t nbytes);
void nmf_model_destroy(nmf_model* model);

/* out[0..9] = nq, nv, nu, nbody, nseg, ngeom, nsite, max_contacts, nsensordata, is_star */
int nmf_model_dims(const nmf_model* model, int32_t out[10]);

/* The most contacts the model's contact set can make in one step (capsules: two end spheres, hulls: up to four vertices;
 * over a terrain with side faces one face contact more per probe).  The engine keeps at most 48 per world (out[7] of
 * nmf_model_dims).  Negative on error. */
int nmf_model_contact_bound(const nmf_model* model);

/* Allocate the state of n_worlds identical worlds on `device` and reset them to the model's
 * "neutral" keyframe.  Replaces: mjw.put_data(nworld=...)  (warp/simulation.py:418-424).
 * NOT stream-ordered (allocations, uploads, one synchronising reset).
 * A model compiled with option/noslip_iterations > 0 (the reference's CPU class: mujoco_globals.yaml:15 under mujoco.mj_step,
 * simulation.py:74-76) runs that friction-only post-pass on every step in contact — the engine of flygym_amd.Simulation, meant for
 * ONE world: the batch then also allocates the pass's scratch, 198 x 200 floats = 158 400 bytes PER WORLD (4096 worlds: 649 MB;
 * nmf_batch_info out[12] says whether), and a step that takes the primal path costs one articulated-body solve per constraint row more.  The
 * reference's batched class strips the option before it compiles the model (warp/simulation.py:427-448) and so does
 * flygym_amd.HIPSimulation; a C caller that wants the batched semantics compiles its model with noslip_iterations = 0. */
nmf_batch* nmf_batch_create(const nmf_model* model, int n_worlds, int device);
void nmf_batch_destroy(nmf_batch* batch);
int nmf_batch_n_worlds(const nmf_batch* batch);

/* The same with explicit options (NULL = defaults = nmf_batch_create).  Every field: 0 = the library's default.  These are the
 * switches the tests and A/B measurements use; none changes WHAT is computed beyond solver tolerance (`solver`) — `sched`,
 * `order`, `max_chunks`, `chunk_div`, `min_chunk_steps`, `order_every` never change a result (worlds are independent).
 * The library reads NO environment variable unless NMF_ALLOW_ENV=1 is set in the process environment (development: the
 * NMF_SOLVER / NMF_SCHED / NMF_ORDER / NMF_MAX_CHUNKS / NMF_CHUNK_DIV / NMF_MIN_CHUNK_STEPS / NMF_ORDER_EVERY /
 * NMF_DISABLE_REST_FAST variables then override these options); what a batch actually runs is reported by nmf_batch_info. */
typedef struct nmf_batch_options {
  int32_t struct_size;      /* sizeof(nmf_batch_options) as the caller was compiled                                            */
  int32_t solver;           /* bit 0: every step on the primal Newton loop; bit 1: the contact-space solve starts from the start
                               point's own sign pattern, not from the previous step's active set; bit 2: its ends are never
                               re-solved on the primal loop (no residual test)                                                 */
  int32_t sched;            /* 1: whole-launch work items (no chunks)                                                          */
  int32_t order;            /* world order of over-subscribed launches: 1 in index order (order kernel), 2 costliest first,
                               3 none (no order kernel), 4 the measured policy of rounds 1-2                                    */
  int32_t max_chunks;       /* 1..16                                                                                           */
  int32_t min_chunk_steps;  /* >= 1                                                                                            */
  int32_t order_every;      /* costliest-first order recomputed every n-th launch                                              */
  int32_t rest_slow;        /* 1: hybrid kernels use the table-driven level passes of the rest of the body                     */
  float chunk_div;          /* each chunk takes 1 / chunk_div of the steps that are left (> 1)                                 */
  int32_t flies_per_cu;     /* > 0: at most this many of the stepping kernel's single-wave workgroups per CU (the kernel's own
                               residency is the ceiling): the launch carries that much idle LDS per workgroup, which leaves LDS and
                               vector registers of every CU to a kernel of ANOTHER stream — the eye renderer of the previous vision
                               tick beside the next tick's physics (co-residency)                          */
} nmf_batch_options;
nmf_batch* nmf_batch_create_ex(const nmf_model* model, int n_worlds, int device, const nmf_batch_options* options);

/* What the batch runs — so that a result can always be traced to the code that made it:
 * out[0] kernel family (0 LEGS_ONLY star, 1 LEGS_ACTIVE_ONLY star, 2 / 3 general tree 144 / 216 dofs, 4 ALL_BIOLOGICAL hybrid,
 * 5 ALL_POSSIBLE hybrid), out[1] terrain kernel, out[2] tether (weld) kernel, out[3] contact-space solve (0 none: primal loop
 * only, 1 star flavour, 2 hybrid flavour), out[4] contacts it takes (steps with more go to the primal loop), out[5] flies
 * (workgroups) per CU, out[6] resident workgroups of the device, out[7] chunked launches (0 / 1), out[8] max chunks,
 * out[9] 1000 * chunk_div, out[10] world-order policy (0 in order, 1 costliest first, 2 none, 3 auto, -1 measured), out[11]
 * solver option bits in effect, out[12] noslip iterations (> 0: the CPU class's flavour — the batch holds 158 400 bytes of noslip
 * scratch per world, see nmf_batch_create), out[13] contact capacity, out[14] LDS bytes / out[15] vector registers of the
 * stepping kernel (from the loaded code object). */
int nmf_batch_info(const nmf_batch* batch, int32_t out[16]);

/* Contacts kept per world and step: min(max_contacts, 48); returns the capacity in effect (negative on error).  Contacts
 * beyond it, in geom order, are dropped and the step counts as overflowed (stats column 2, nmf_stats overflow steps).
 * Call between launches (synchronous).  Replaces: the nconmax of mjw.put_data  (warp/simulation.py:50-56, 418-424). */
int nmf_batch_set_contact_capacity(nmf_batch* batch, int max_contacts);

/* Reset every world to the neutral keyframe (qpos, ctrl from the keyframe; qvel = 0; time = 0)
 * and refresh the pose outputs.  Replaces GPUSimulation.reset (warp/simulation.py:64-71). */
int nmf_reset(nmf_batch* batch, void* stream);

/* Same for the worlds with mask_dev[w] != 0 only (uint8 per world, device memory); the others keep their state and
 * their own clock.  No reference counterpart (its reset re-uploads every world): episode resets for RL loops. */
int nmf_reset_worlds(nmf_batch* batch, const uint8_t* mask_dev, void* stream);

/* Advance all worlds by n_steps physics steps in ONE kernel launch, controls held constant.
 * Replaces n_steps calls of GPUSimulation.step (warp/simulation.py:260-263). */
int nmf_step(nmf_batch* batch, int n_steps, void* stream);

/* Same, but before step s the controls ctrl[w][act_ids[a]] are loaded from
 * table[w][(start + s) % table_steps][a]  (a < n_act): the device-resident kinematic-replay
 * loop of the reference benchmark (src/flygym_demo/benchmark/time_gpu_simulation.py:137-150:
 * update_target_angles_kernel + set_actuator_inputs + step + increment_counter, graph-captured). */
int nmf_step_replay(nmf_batch* batch, const float* table_dev, int table_steps, int n_act,
                    const int32_t* act_ids_dev, int start, int n_steps, void* stream);

/* The same launch (table_dev NULL: nmf_step, controls held; else nmf_step_replay with n_act_table columns) that also RECORDS the
 * observation block after every obs_every-th step — what the reference's loops read after every step (get_joint_angles /
 * get_joint_velocities / get_actuator_forces / get_ground_contact_info, src/flygym/simulation.py:142-243; MJWarp computes its
 * sensors every step, warp/simulation.py:260-263), without leaving the kernel:
 *   ring[(s + 1) / obs_every - 1][w][0 .. 2 n_joint + n_act + 96) for every step s (0-based) with (s + 1) % obs_every == 0,
 * in the layout of nmf_pack_observations — [joint angles | joint velocities | forces of the first n_act actuators | the 96
 * contact-sensor floats] — and with its values: each row is bit for bit what nmf_pack_observations gives when the launch ends at
 * that step.  ring_dev: float32 [n_steps / obs_every][n_worlds][row_stride].  The contact sensors and actuator forces are
 * evaluated on the recorded steps (and, as always, on the launch's last step for the batch's own arrays).
 * n_steps must be a multiple of obs_every (a trailing partial window would be stepped but never recorded: refused). */
int nmf_step_record(nmf_batch* batch, const float* table_dev, int table_steps, int n_act_table, const int32_t* act_ids_dev, int start,
                    int n_steps, int obs_every, int n_joint, int n_act, float* ring_dev, int row_stride, void* stream);

/* Device pointer + row width of a per-world field (zero-copy views for PyTorch). */
float* nmf_field_ptr(nmf_batch* batch, int field, int32_t* width);

/* dst[w][k] = field[w][ids[k]*group .. +group)  — gather in caller order (group = 1, 3 or 4).
 * Replaces wp_gather_indexed_cols_2d / _rows_vec3f / _rows_quatf (warp/utils.py:29-127). */
int nmf_gather(nmf_batch* batch, int field, const int32_t* ids_dev, int n_ids, int group,
               float* dst_dev, void* stream);

/* field[w][ids[k]] = src[w][k]  — scatter controls in caller order.
 * Replaces wp_scatter_indexed_cols_2d (warp/utils.py:84-104). */
int nmf_scatter(nmf_batch* batch, int field, const int32_t* ids_dev, int n_ids,
                const float* src_dev, void* stream);

/* The observation block of the multi-GPU exchange, packed in ONE launch: out[w][0 .. 2 n_joint + n_act + 96) =
 * [joint angles (qpos 7 ..) | joint velocities (qvel 6 ..) | forces of the first n_act actuators | the 96 contact-sensor
 * floats], rows row_stride floats apart.  Replaces the four getter launches the reference would need per tick
 * (get_joint_angles / get_joint_velocities / get_actuator_forces / contact sensors, warp/simulation.py:73-211) as the
 * input of the RCCL all-gather (flygym_amd.sharding.ObsGather; the reference is single-GPU, warp/utils.py:192-202). */
int nmf_pack_observations(nmf_batch* batch, int n_joint, int n_act, float* out_dev, int row_stride, void* stream);

/* Number of physics steps taken since the last reset (host-side counter, no sync). */
int64_t nmf_step_count(const nmf_batch* batch);

/* Timing helper for benchmarks: runs nmf_step/nmf_step_replay `reps` times on `stream`
 * bracketed by hipEvents recorded on that same stream; returns mean milliseconds per launch
 * (blocks the host).  table_dev may be NULL for constant controls. */
double nmf_time_launches(nmf_batch* batch, const float* table_dev, int table_steps, int n_act,
                         const int32_t* act_ids_dev, int n_steps, int reps, void* stream);

/* Measurement helper: the shader clock the stepping kernel actually ran at.  Workgroup 0 of every stepping launch reads
 * the shader-cycle counter (s_memtime) and the constant 100 MHz counter (s_memrealtime) when it starts and when it
 * ends; the library accumulates both differences.  *hz_out = 1e8 * (shader cycles) / (100 MHz ticks) over the launches
 * since the last call with reset != 0 (0 if there were none).  Synchronises with the device.  No reference
 * counterpart: bench.py prices the kernel's instruction issue against the clock of the run it measures. */
int nmf_shader_clock(nmf_batch* batch, double* hz_out, int reset);

/* ---- sensors the north star names; the reference snapshot holds only their constants
 * (src/flygym/assets/model/legacy/flygym1_config.yaml:141-192), so semantics are build-defined. ---- */

/* Hex-ommatidia resample of raw eye images.  images[n_images][n_pixels][3] uint8 RGB; id_map[n_pixels] 16-bit:
 * bits 0..14 = 0 (no ommatidium) or k (ommatidium k-1), bit 15 = that ommatidium is pale; shared by all images;
 * pale[n_ommatidia] uint8 (1 = pale type, reads blue; 0 = yellow type, reads green); inv_norm[k] = 1 / (255 * pixels of ommatidium k);
 * out[n_images][n_ommatidia][2] float32 (channel 0 yellow, 1 pale).  Buffers 16-byte aligned.
 * plan: NULL, or the run plan of the id map written by nmf_retina_plan into a buffer of nmf_retina_plan_bytes(n_pixels)
 * bytes (16 bytes per 16-pixel chunk, then the list of chunks that touch an ommatidium): with a plan
 * and n_pixels a multiple of 1024 the frames are streamed with fully coalesced loads; the results
 * are identical either way (integer sums). */
size_t nmf_retina_plan_bytes(int n_pixels);
int nmf_retina_plan(const int16_t* id_map_dev, int n_pixels, void* plan_dev, void* stream);
int nmf_retina_resample(const uint8_t* images_dev, const int16_t* id_map_dev, const void* plan_dev, const uint8_t* pale_dev,
                        const float* inv_norm_dev, int n_images, int n_pixels, int n_ommatidia,
                        float* out_dev, void* stream);

/* Compound-eye renderer fused with the ommatidia resample (no reference counterpart in this snapshot: the eye cameras,
 * like the resample, survive only as constants in src/flygym/assets/model/legacy/flygym1_config.yaml:141-173; the
 * reference's image path is rendering.py / warp/rendering.py -> MuJoCo / MJWarp renderers).  Build-defined (DESIGN.md
 * section 7): each eye is an equidistant-fisheye camera attached to a body segment; the scene is the ground (checker
 * plane, or the terrain relief of the batch's world), a uniform sky, up to 8 spheres and the fly's own body as up to 64
 * capsules rigidly attached to segments (what reference warp/rendering.py:385-441 gives the batch renderer: the whole
 * model).  Reads the segment poses of the last nmf_step / nmf_reset. */
typedef struct nmf_eye_params {
  int32_t height, width;        /* raw frame size in pixels; height * width a multiple of 16                           */
  float fov_deg;                /* full angle seen along the vertical image axis (ray angle is proportional to radius)   */
  int32_t eye_seg[2];           /* parent segment of each eye camera (index into the batch's segment order)             */
  float rel_pos[2][3];          /* camera position in the parent segment frame                                           */
  float rel_quat[2][4];         /* camera orientation in the parent frame (w,x,y,z); the camera looks along -z, +y is up */
  float checker_size;           /* side of a ground checker square                                                       */
  uint8_t sky_rgb[4], ground_rgb[2][4], sphere_rgb[8][4];   /* colours (4th byte unused)                                */
  int32_t n_spheres;            /* 0..8                                                                                  */
  int32_t spheres_per_world;    /* 1: spheres_dev is [n_worlds][n_spheres][4]; 0: [n_spheres][4] shared by all worlds   */
  uint8_t wall_rgb[4], body_rgb[4];   /* side walls of the terrain relief; the fly's own body                          */
  int32_t n_capsules;           /* 0..64 capsules of the fly's own body (capsule_seg_dev / capsule_geom_dev)            */
  int32_t terrain_relief;       /* 1: the ground is the height map the batch's physics collides with (gapped / blocks /
                                   mixed worlds: constant-height cells with side walls); 0: the flat checker plane      */
  int32_t rays_per_ommatidium;  /* 0: every pixel of the raw frame that lies in an ommatidium's cell is cast (readings =
                                   resampling the rendered frame, bit for bit); 16: sixteen of each cell's pixels — at
                                   indices floor((2 j + 1) n / 32) of its n pixels in raster order — and the reading is
                                   their mean: 15 x fewer rays, an approximation of the cell mean (no frames in this mode) */
} nmf_eye_params;

/* sizeof(nmf_eye_params) as this library was compiled: lets a foreign-language binding verify its struct layout. */
size_t nmf_eye_params_size(void);

/* The visit plan of the renderer: which 16-pixel chunks feed an ommatidium, in which order, with the bounding cones of their rays,
 * the sampled mode's pixel lists — and the plan's OWN device copies of the id map, the retina run plan (nmf_retina_plan), the pale
 * flags and the normalisation, so that later changes to the caller's buffers cannot reach a render.  nmf_eye_plan_create is NOT
 * stream-ordered and must not be called inside a stream capture: it synchronises the device, copies the id map / run plan / pale
 * flags to the host, sorts there, allocates and uploads (tens of milliseconds, once per id map and lens).  The plan belongs to the
 * device it was made on and to no batch: any batch on that device can render with it.  NULL on error (nmf_last_error). */
nmf_eye_plan* nmf_eye_plan_create(const int16_t* id_map_dev, const void* plan_dev, const uint8_t* pale_dev, const float* inv_norm_dev,
                                  int height, int width, float fov_deg, int n_ommatidia, int device);
void nmf_eye_plan_destroy(nmf_eye_plan* plan);

/* Render with an explicit plan: argument checks and ONE kernel launch — stream-ordered, hipGraph-capturable (a vision tick =
 * nmf_step + nmf_eye_render_planned captures as one graph).  params->height / width / fov_deg must be the plan's. */
int nmf_eye_render_planned(nmf_batch* batch, const nmf_eye_params* params, const nmf_eye_plan* plan, const float* spheres_dev,
                           const int32_t* capsule_seg_dev, const float* capsule_geom_dev, uint8_t* frames_out_dev, float* omm_out_dev,
                           void* stream);

/* The same without a handle: the batch builds a plan on the first call with a new (id_map_dev, plan_dev, pale_dev, inv_norm_dev,
 * shape, lens) — keyed on the buffer ADDRESSES — and keeps up to four of them (least recently used first out).  That first call
 * is therefore NOT stream-ordered (see nmf_eye_plan_create) and not capturable; later calls with the same key are.  The plan holds
 * copies: a caller that rewrites one of the four buffers in place keeps rendering with the old contents until it passes other
 * addresses — use the explicit handle where that matters.
 * spheres_dev: (x, y, z, radius) per sphere, float32.  id_map / plan / pale / inv_norm as for nmf_retina_resample (the
 * plan is required).  frames_out_dev: NULL or uint8 [n_worlds][2][height*width][3] raw eye frames;
 * omm_out_dev: NULL or float32 [n_worlds][2][n_ommatidia][2].  Rendering frames and resampling them with
 * nmf_retina_resample gives bit-identical ommatidia readings (integer sums).
 * capsule_seg_dev[n_capsules] int32 segment index, capsule_geom_dev[n_capsules][7] float32 (end points p0, p1 in the
 * segment frame, radius) — NULL when n_capsules is 0. */
int nmf_eye_render(nmf_batch* batch, const nmf_eye_params* params, const float* spheres_dev,
                   const int32_t* capsule_seg_dev, const float* capsule_geom_dev, const int16_t* id_map_dev, const void* plan_dev, const uint8_t* pale_dev, const float* inv_norm_dev,
                   int n_ommatidia, uint8_t* frames_out_dev, float* omm_out_dev, void* stream);

/* Batch camera renderer for selected worlds of a batch: the camera a person looks through.  Replaces the reference's
 * WarpGPUBatchRenderer (warp/rendering.py:279-341: mjw.create_render_context once, then mjw.refit_bvh + mjw.render +
 * get_rgb_selected_worlds_and_cameras per frame; attached by GPUSimulation.set_renderer, warp/simulation.py:266-342).
 * Build-defined (specification tests/camera_spec.py): pinhole cameras — pixel (row, col) has the
 * camera-frame ray (u, -v, -1) normalised, u = (col + 0.5 - W/2) t, v = (row + 0.5 - H/2) t, t = tan(fovy/2) / (H/2);
 * x right, y up, looking along -z — the eye renderer's scene plus the whole fly as capsules with a colour each, one
 * directional light from straight above: colour = base * (ambient + diffuse * max(0, n_z)), rounded to uint8.
 * Reads the segment poses of the last nmf_step / nmf_reset. */
#define NMF_CAMERA_MAX 8          /* cameras per plan */
#define NMF_CAMERA_MAX_CAPSULES 72
#define NMF_CAMERA_FIXED 0        /* pos and rot are world coordinates                                                   */
#define NMF_CAMERA_TRACK 1        /* position = position of segment track_seg + pos; orientation constant in the world
                                     (MuJoCo's "track" for a camera whose parent is that segment)                        */
typedef struct nmf_camera_view {
  int32_t mode;                 /* NMF_CAMERA_FIXED / NMF_CAMERA_TRACK                                                   */
  int32_t track_seg;            /* tracked segment (index into the batch's segment order); ignored for fixed cameras    */
  float fovy_deg;               /* full vertical field of view, 0 < fovy < 180                                          */
  float pos[3];                 /* world position (fixed) or offset from the tracked segment (track)                    */
  float rot[9];                 /* camera axes in the world, row-major, columns right / up / back (orthonormal)        */
} nmf_camera_view;

typedef struct nmf_camera_params {
  int32_t height, width;        /* frame size in pixels, each >= 1                                                       */
  nmf_camera_view cam[NMF_CAMERA_MAX];
  float ambient, diffuse;       /* light terms                                                                           */
  float checker_size;           /* the nmf_eye_params scene fields, with the same meaning                               */
  uint8_t sky_rgb[4], ground_rgb[2][4], sphere_rgb[8][4];
  int32_t n_spheres, spheres_per_world;
  uint8_t wall_rgb[4];
  int32_t terrain_relief;
} nmf_camera_params;

/* sizeof(nmf_camera_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_camera_params_size(void);

/* Replaces WarpGPUBatchRenderer._render_setup_impl (warp/rendering.py:282-309: the world / camera id arrays and
 * mjw.create_render_context).  An explicit handle: takes HOST arrays — params, world_ids[n_selected] (each in
 * [0, n_worlds), distinct), cap_seg[n_caps] (< the batch's segment count), cap_geom[n_caps][7] (end points p0, p1 in the
 * segment frame, radius), cap_rgb[n_caps][3] — validates them, and owns device copies.  1 <= n_cameras <= NMF_CAMERA_MAX,
 * 0 <= n_caps <= NMF_CAMERA_MAX_CAPSULES, n_selected >= 1.  NOT stream-ordered (allocations and synchronous uploads, once);
 * must not be called inside a stream capture.  The plan belongs to the batch it was made for.  NULL on error (nmf_last_error). */
nmf_camera_plan* nmf_camera_plan_create(nmf_batch* batch, const nmf_camera_params* params, int n_cameras,
                                        const int32_t* world_ids, int n_selected, const int32_t* cap_seg, const float* cap_geom,
                                        const uint8_t* cap_rgb, int n_caps);
void nmf_camera_plan_destroy(nmf_camera_plan* plan);

/* Replaces WarpGPUBatchRenderer._render_impl (warp/rendering.py:311-321).  Argument checks and ONE kernel launch on
 * `stream` (the stream the batch is stepped on): no allocation, no host synchronisation, hipGraph-capturable — nmf_step +
 * nmf_camera_render capture as one graph.  spheres_dev: NULL when the plan has no spheres, else float32 (x, y, z, radius)
 * [n_spheres][4], or [n_worlds][n_spheres][4] with spheres_per_world = 1.  frames_out_dev: uint8
 * [n_selected][n_cameras][height][width][3], 16-byte aligned. */
int nmf_camera_render(nmf_batch* batch, const nmf_camera_plan* plan, const float* spheres_dev, uint8_t* frames_out_dev, void* stream);

/* The same renderer for a world with several flies (reference GPUSimulation.set_renderer draws the whole world, every fly in
 * it).  One batch per fly (flygym_amd.simulation.MultiFlyHIPSimulation), all of the same n_worlds on one device, world w of
 * every batch being the same world.  Fly f's capsules take their poses from batch f.  Compositing: the nearest hit wins; on an
 * exact tie the earlier object does — ground / terrain, spheres, then capsules in the order (fly, capsule) — which is
 * tests/camera_spec.py with the flies' capsules concatenated. */
#define NMF_CAMERA_MAX_FLIES 4    /* flies per plan, each with at most NMF_CAMERA_MAX_CAPSULES capsules */
typedef struct nmf_camera_fly {
  nmf_batch* batch;             /* the batch that steps this fly                                                         */
  const int32_t* cap_seg;       /* HOST arrays as for nmf_camera_plan_create: [n_caps], < this batch's segment count     */
  const float* cap_geom;        /* [n_caps][7]                                                                           */
  const uint8_t* cap_rgb;       /* [n_caps][3]                                                                           */
  int32_t n_caps;               /* 0 <= n_caps <= NMF_CAMERA_MAX_CAPSULES                                                */
} nmf_camera_fly;

/* nmf_camera_plan_create for 1 <= n_flies <= NMF_CAMERA_MAX_FLIES flies.  cam_fly[n_cameras]: the fly (index into `flies`)
 * whose batch a NMF_CAMERA_TRACK camera follows — its track_seg is a segment of THAT batch; ignored for fixed cameras but
 * must be in range.  Every check of nmf_camera_plan_create, and: every batch non-null, all on one device, of equal n_worlds,
 * with the same z-up ground plane and the same terrain kind and parameters.  The plan owns device copies of everything; it
 * belongs to these batches, which must outlive it.  NOT stream-ordered.  NULL on error (nmf_last_error). */
nmf_camera_plan* nmf_camera_plan_create_flies(const nmf_camera_fly* flies, int n_flies, const nmf_camera_params* params,
                                              const int32_t* cam_fly, int n_cameras, const int32_t* world_ids, int n_selected);

/* nmf_camera_render for a plan of nmf_camera_plan_create_flies: argument checks and ONE kernel launch on `stream`, which
 * must be ordered after the last step of every batch of the plan (the batches of a MultiFlyHIPSimulation are stepped on one
 * stream).  No allocation, no host synchronisation, hipGraph-capturable as a single node.  Arguments as nmf_camera_render. */
int nmf_camera_render_flies(const nmf_camera_plan* plan, const float* spheres_dev, uint8_t* frames_out_dev, void* stream);

/* Closed-loop steerable tripod CPG with its state on the device (flygym_amd.controllers.TurningCPG; csrc/nmf_cpg.hip).  No
 * reference counterpart: the snapshot has no CPG (flygym 2.0.1 dropped flygym 1.x's controllers), so this is build-defined
 * (specification tests/cpg_spec.py).  Per world six coupled phase oscillators, legs in the order lf lm lh
 * rf rm rh (side = leg / 3, tripod phase bias b = pi * (leg & 1)): phase theta in cycles in [0, 1) (float64), magnitude r
 * (float32), and an input drive d = (d_left, d_right) (float32).  One step at dt = timestep writes one table row from the state
 * BEFORE its update, and every right-hand side uses the old state:
 *   x = theta_l n_bins, i0 = floor(x) mod n_bins, f = x - floor(x), c = (1 - f) cycle[i0][col] + f cycle[(i0 + 1) mod n_bins][col]
 *   row[col] = c + (r_l - 1) (c - mean[col])   (l = leg_of_col[col]; mean = the cycle's mean over its bins; r = 1: c itself)
 *   row[n_pos + l] = stance[i0][l] ? adhesion_on : adhesion_off        (the six optional columns)
 *   theta_l <- (theta_l + dt (frequency sign(d_side) + (1 / 2 pi) sum_{j != l} r_j coupling sin(2 pi (theta_j - theta_l) - (b_j - b_l)))) mod 1
 *   r_l     <- r_l + dt convergence (|d_side| - r_l)                   (sign(0) = 0: that side holds its phase)
 * The phase, x and the phase increment are float64, everything else float32; the magnitudes' Euler sums are kept in float64
 * beside the float32 array the formulas read (a magnitude the caller writes takes effect at the next launch). */
typedef struct nmf_cpg_params {
  int32_t n_pos;                /* position-target columns of a row (1..4096)                                            */
  int32_t n_bins;               /* phase bins of the step cycle (>= 2)                                                   */
  double frequency;             /* Hz at |drive| > 0                                                                     */
  double timestep;              /* seconds per step (the batch's physics timestep)                                       */
  float coupling;               /* weight w of every pair                                                                */
  float convergence;            /* rate a of the magnitudes                                                              */
  float adhesion_on, adhesion_off;   /* values of the adhesion columns in stance / swing (used with stance bins only)   */
  int32_t table_steps;          /* rows per world of the tables nmf_cpg_advance will be given (>= 1)                     */
} nmf_cpg_params;

/* sizeof(nmf_cpg_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_cpg_params_size(void);

/* An explicit handle for the worlds of `batch`, on its device: takes HOST arrays — cycle[n_bins][n_pos] float32,
 * leg_of_col[n_pos] (each in 0..5), stance[n_bins][6] uint8 or NULL (NULL: rows of n_pos columns; else n_pos + 6) — validates
 * them, owns device copies and the state arrays, and resets every world (nmf_cpg_reset with first_world 0 of n_worlds).  NOT
 * stream-ordered (allocations, synchronous uploads); must not be called inside a stream capture.  NULL on error
 * (nmf_last_error): n_bins < 2, a leg_of_col outside 0..5, ... */
nmf_cpg* nmf_cpg_create(nmf_batch* batch, const nmf_cpg_params* params, const float* cycle, const int32_t* leg_of_col,
                        const uint8_t* stance);
void nmf_cpg_destroy(nmf_cpg* cpg);

/* The worlds with mask_dev[w] != 0 (uint8 per world, device memory; NULL: all) get theta_l = ((first_world + w) / total_worlds +
 * b_l / 2 pi) mod 1, r = 1, drive = (1, 1): the tripod, world by world one gait cycle apart — first_world / total_worlds place
 * a shard inside a larger (multi-GPU) population, as TripodCPG.targets does.  The others keep their state.  Stream-ordered. */
int nmf_cpg_reset(nmf_cpg* cpg, const uint8_t* mask_dev, int first_world, int total_worlds, void* stream);

/* Device pointer + row width of a per-world array of the controller (zero-copy views; writable between launches). */
#define NMF_CPG_PHASE 0           /* [6] float64, cycles in [0, 1) */
#define NMF_CPG_MAGNITUDE 1       /* [6] float32                   */
#define NMF_CPG_DRIVE 2           /* [2] float32 (left, right)     */
#define NMF_CPG_RETRACTION 3      /* [6] float32 rho in [0, max_correction]            (after nmf_cpg_hybrid_enable) */
#define NMF_CPG_STUMBLING 4       /* [6] float32 sigma in [0, max_correction]          (after nmf_cpg_hybrid_enable) */
#define NMF_CPG_RULE_FLAGS 5      /* [6] uint8: bit 0 retract, bit 1 stumble, of the last hybrid launch (after enable) */
void* nmf_cpg_field_ptr(nmf_cpg* cpg, int which, int32_t* width);

/* Advance every world by n_steps and write table_dev[w][s][0 .. n_act) for s < n_steps (float32 [n_worlds][table_steps][n_act],
 * n_act = n_pos or n_pos + 6: the table of nmf_step_replay / nmf_step_record with start = 0); rows n_steps .. table_steps - 1
 * are not touched.  The drive is read when the launch starts.  Argument checks and ONE kernel launch on `stream`: no allocation,
 * no host synchronisation, hipGraph-capturable.  Refused: a null table, table_steps other than the params', n_steps outside
 * 1..table_steps, a table on another device than the controller's (checked outside stream captures). */
int nmf_cpg_advance(nmf_cpg* cpg, int n_steps, float* table_dev, int table_steps, void* stream);

/* The hybrid controller: the CPG above plus two sensory rules that lift a leg (flygym_amd.controllers.HybridTurningCPG;
 * specification tests/hybrid_spec.py).  Build-defined and pinned by nothing, like the CPG: the rules are this project's statement
 * of flygym 1.x's hybrid controller, the default constants are flygym 1.x's as remembered.  State per world
 * and leg beside the CPG's: retraction rho and stumbling sigma (float32, >= 0).  The decision is taken ONCE per launch, from the
 * batch's seg_xpos / seg_xquat / sensordata as they stand when the launch starts (the last step of the previous launch):
 *   h_l = z(root segment) - z(tip segment of leg l); L = the leg of the largest h (ties: the lowest index); h3 = the third largest h
 *   retract[L]  = h_L > h3 + retraction_threshold                                          (at most one leg per world)
 *   stumble[l]  = swing[i0_l][l] and found_l > 0 and F_l . xhat < -stumbling_force_threshold
 * i0_l: the leg's phase bin when the launch starts; xhat: the root segment's x axis in the world; F_l: the leg's net sensor force in
 * the world frame (rebuilt from the reported normal n and tangent t1, third axis n x t1, where the model's semantics report it in
 * the contact frame).  Per step, flags held for the launch, the row from the state before its update:
 *   net_l = rho_l > 0 ? rho_l : sigma_l
 *   row[col] = fl(row of the CPG + fl(net_l corr[col]))          (two float32 roundings, no fused multiply-add)
 *   row[n_pos + l] = adhesion_off while net_l > 0                (with the six adhesion columns)
 *   rho_l   <- retract[l] ? min(rho_l + dt retraction_up, max_correction)  : max(rho_l - dt retraction_down, 0)
 *   sigma_l <- stumble[l] ? min(sigma_l + dt stumbling_up, max_correction) : max(sigma_l - dt stumbling_down, 0)
 * with the four increments rounded to float32 once.  The oscillators are not modified by the rules. */
typedef struct nmf_cpg_hybrid_params {
  float retraction_threshold;        /* in the model's length unit (>= 0)                      */
  float stumbling_force_threshold;   /* in the sensor's force unit (>= 0)                      */
  float retraction_up, retraction_down;     /* rates of rho per second (>= 0)                  */
  float stumbling_up, stumbling_down;       /* rates of sigma per second (>= 0)                */
  float max_correction;              /* the cap of rho and sigma (>= 0)                        */
} nmf_cpg_hybrid_params;

/* sizeof(nmf_cpg_hybrid_params) as this library was compiled. */
size_t nmf_cpg_hybrid_params_size(void);

/* Switch the rules on for this controller, once: takes HOST arrays — corr[n_pos] float32 (radians per unit of net, per position
 * column), swing[n_bins][6] uint8 — and the indices, in the batch's segment order, of the root segment and of the six legs' tip
 * segments; validates them and allocates rho, sigma and the flags, zeroed.  NOT stream-ordered (allocations, synchronous uploads);
 * must not be called inside a stream capture.  Refused (nmf_last_error): a second call, a segment index outside the batch's segment
 * count, a negative or non-finite rate / cap / threshold, a non-finite corr, a batch whose model has no leg sensors (or whose
 * sensordata is not the six leg sensors' 96 values); a refused call leaves the controller as it was.  The controller keeps
 * pointers to the batch's seg_xpos / seg_xquat / sensordata arrays: the batch must outlive the controller (destroy the
 * controller first), and nmf_cpg_advance_hybrid after the batch is gone reads freed memory. */
int nmf_cpg_hybrid_enable(nmf_cpg* cpg, const nmf_cpg_hybrid_params* params, const float* corr, const uint8_t* swing, int root_seg,
                          const int32_t tip_seg[6]);

/* nmf_cpg_advance with the rules: reads the batch's seg_xpos / seg_xquat / sensordata itself, writes the launch's flags
 * (NMF_CPG_RULE_FLAGS) and advances rho / sigma with the oscillators.  Argument checks and ONE kernel launch on `stream`: no
 * allocation, no host synchronisation, hipGraph-capturable.  Refused: a controller without nmf_cpg_hybrid_enable, and everything
 * nmf_cpg_advance refuses.  nmf_cpg_reset also zeroes rho / sigma / flags of the masked worlds once the rules are enabled. */
int nmf_cpg_advance_hybrid(nmf_cpg* cpg, int n_steps, float* table_dev, int table_steps, void* stream);

/* Advected odor plumes with their state on the device (flygym_amd.sensors.OdorPlume; csrc/nmf_plume.hip).  No reference
 * counterpart: the snapshot holds no plume code and no plume data (flygym 1.x replayed one recording of an offline fluid simulation
 * to one fly), so the whole model is build-defined and pinned by nothing (specification tests/plume_spec.py).
 * A plume is a float32 concentration grid c[height][width] over the ground plane: cell (j, i) is centred at
 * (origin_x + (i + 1/2) cell_size, origin_y + (j + 1/2) cell_size), and cells outside the grid read as 0 everywhere below (clean
 * air flows in, odor flows out).  A handle holds n_plumes of them — 1 (every world smells the same plume) or the batch's n_worlds —
 * each with two grids (ping and pong), a wind w = (wx, wy) float32 and a tick counter (uint32); WHICH grid is current is one parity
 * word in device memory, read by every kernel and flipped by every tick.  One tick of tick_s seconds, every cell from the old grid:
 *   v = w + eddy_gain E[j][i]                                  (E[height][width][2]: optional static eddies, shared by all plumes)
 *   d = vx r, k = floor(d), f = d - k; (l, g) likewise from vy (r = tick_s / cell_size: any displacement is legal, no CFL clamp)
 *   adv = (1 - g) ((1 - f) c[j-l][i-k] + f c[j-l][i-k-1]) + g ((1 - f) c[j-l-1][i-k] + f c[j-l-1][i-k-1])
 *   dif = D (c[j][i-1] + c[j][i+1] + c[j-1][i] + c[j+1][i] - 4 c[j][i])             (D = diffusivity tick_s / cell_size^2)
 *   c_new[j][i] = max(adv + dif, S[j][i])                      (S[height][width]: the source map, shared by all plumes)
 * and then, per plume, one Ornstein-Uhlenbeck step of the wind and tick <- tick + 1:
 *   w <- (w + a (mean_wind - w)) + b xi        a = tick_s / wind_tau, b = wind_sigma sqrt(tick_s); per component
 *   xi = ((u0 + u1) + (u2 + u3) - 2) sqrt(3),  u_m = (hash(x_m) >> 8) 2^-24,
 *   x_m = seed ^ (world 0x9E3779B9) ^ (tick 0x85EBCA6B) ^ (m 0xC2B2AE35)   (uint32; m = 0..3 for x, 4..7 for y; tick: before its increment)
 *   hash(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 * world = first_world + the plume's index (the placement of a shard inside a larger population, as nmf_cpg_reset's).  r, D, a and
 * b are computed in float64 and rounded to float32 once; the grid, wind and reading arithmetic is float32 with every operation rounded
 * as written above (no contraction, no reassociation; the reading's division correctly rounded).  The diffusion term is taken at
 * the cell, not at its upstream point: a wind within 2 D cells of an odd whole number of cells per tick amplifies cell-to-cell
 * stripes, and the concentration may exceed the source's peak.  wind_sigma = 0 gives a deterministic wind; the caller may overwrite the wind between
 * launches (NMF_PLUME_WIND).  Every cell is written by one lane from the old grid alone (no atomics): results are bitwise
 * reproducible from run to run.
 * A reading at the point (x, y) is the current grid interpolated bilinearly between cell centres, times intensity_scale:
 *   u = (x - origin_x) / cell_size - 1/2, i0 = floor(u), f = u - i0; (v, j0, g) likewise from y
 *   reading = intensity_scale ((1 - g) ((1 - f) c[j0][i0] + f c[j0][i0+1]) + g ((1 - f) c[j0+1][i0] + f c[j0+1][i0+1]))
 * so it falls to 0 continuously at the border; a point with u outside [-1/2, width - 1/2] or v outside [-1/2, height - 1/2] (or
 * not a number) sets its world's out-of-bounds byte. */
typedef struct nmf_plume_params {
  int32_t n_plumes;             /* 1, or the batch's n_worlds                                                            */
  int32_t height, width;        /* cells (8..1024 each)                                                                  */
  int32_t first_world;          /* global index of plume 0 in the noise's world term (>= 0)                              */
  float cell_size;              /* h, in the model's length unit (> 0)                                                   */
  float origin_x, origin_y;     /* the grid's corner of least x and y                                                    */
  float tick_s;                 /* seconds per plume tick (> 0)                                                          */
  float diffusivity;            /* kappa, length^2 per second (>= 0; kappa tick_s / h^2 <= 1/4)                          */
  float mean_wind_x, mean_wind_y;   /* length per second                                                                 */
  float wind_tau;               /* relaxation time of the wind, seconds (> 0)                                            */
  float wind_sigma;             /* noise amplitude of the wind, length per second per sqrt(second) (>= 0)                */
  float eddy_gain;              /* scale of the eddy field (ignored without one)                                         */
  float intensity_scale;        /* factor of every reading                                                               */
  uint32_t seed;
} nmf_plume_params;

/* sizeof(nmf_plume_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_plume_params_size(void);

/* An explicit handle for the worlds of `batch`, on its device: takes HOST arrays — source[height][width] float32 and
 * eddies[height][width][2] float32 or NULL — validates them, owns device copies and the state arrays, and resets every plume
 * (nmf_plume_reset with a NULL mask; parity 0).  NOT stream-ordered (allocations, synchronous uploads); must not be called inside
 * a stream capture.  NULL on error (nmf_last_error): n_plumes other than 1 or the batch's n_worlds; height or width outside
 * 8..1024; kappa tick_s / h^2 > 1/4; a cell_size, tick_s or wind_tau that is not positive; a negative diffusivity, wind_sigma or
 * first_world; a value that is not finite in the params, the source map or the eddies; a NULL source map.  The handle keeps
 * pointers to the batch's seg_xpos / seg_xquat arrays (nmf_plume_sample_sites): destroy it before the batch. */
nmf_plume* nmf_plume_create(nmf_batch* batch, const nmf_plume_params* params, const float* source, const float* eddies);
void nmf_plume_destroy(nmf_plume* plume);

/* The plumes with mask_dev[p] != 0 (uint8 per PLUME, device memory; NULL: all) get both grids zeroed, tick = 0 and w = mean_wind;
 * the others are not touched, and neither is the parity word.  Stream-ordered. */
int nmf_plume_reset(nmf_plume* plume, const uint8_t* mask_dev, void* stream);

/* n_ticks ticks of every plume: argument checks and, per tick, two kernel launches on `stream` (the grids, then winds / tick
 * counters / parity).  No allocation, no host synchronisation, hipGraph-capturable: the kernels find the current grid through the
 * parity word, so a captured advance replays correctly any number of times.  Refused: n_ticks < 1. */
int nmf_plume_advance(nmf_plume* plume, int n_ticks, void* stream);

/* Device pointer + row width of an array of the handle (zero-copy views; writable between launches). */
#define NMF_PLUME_WIND 0          /* [n_plumes][2] float32                                                        */
#define NMF_PLUME_TICKS 1         /* [n_plumes][1] uint32                                                         */
#define NMF_PLUME_GRID0 2         /* [n_plumes][height * width] float32: the current grids while the parity is 0  */
#define NMF_PLUME_GRID1 3         /* [n_plumes][height * width] float32: the current grids while the parity is 1  */
#define NMF_PLUME_PARITY 4        /* ONE int32 word, 0 or 1 (width 1; not per plume)                              */
void* nmf_plume_field_ptr(nmf_plume* plume, int which, int32_t* width);

/* Readings at caller-given points: points_dev[n_worlds][n_pts][2] float32 (x, y) -> out_dev[n_worlds][n_pts] float32, and
 * oob_dev[n_worlds] uint8 = 1 where any of the world's points lies out of bounds (else 0).  World w reads plume w (plume 0 when
 * n_plumes is 1).  Argument checks and ONE kernel launch on `stream`: no allocation, no host synchronisation, capturable.
 * Refused: a null buffer, n_pts < 1. */
int nmf_plume_sample_points(nmf_plume* plume, const float* points_dev, int n_pts, float* out_dev, uint8_t* oob_dev, void* stream);

/* Readings at n_sensors points rigidly attached to segments, placed exactly as nmf_odor_intensity places them (sensor_seg = index
 * into the batch's segment order, clamped to it; sensor_rel = offset in the segment frame; the point is the x, y of seg_xpos +
 * R(seg_xquat) rel, z is ignored): out_dev[n_worlds][n_sensors] float32 and oob_dev[n_worlds] uint8 as above, from the poses of the
 * last nmf_step / nmf_reset.  ONE kernel launch on `stream`, capturable.  Refused: a null buffer, n_sensors < 1. */
int nmf_plume_sample_sites(nmf_plume* plume, const int32_t* sensor_seg_dev, const float* sensor_rel_dev, int n_sensors,
                           float* out_dev, uint8_t* oob_dev, void* stream);

/* Sensory steering (flygym_amd.controllers.SensorySteering; csrc/nmf_taxis.hip): the ommatidia readings of both eyes and the
 * readings of the four odor sites become the CPG's drive (left, right) in ONE launch, with no state and no handle.  No reference
 * counterpart (the snapshot holds no controller and no vision processing): build-defined and pinned by nothing (DESIGN.md section 7,
 * specification tests/taxis_spec.py).  Per world:
 *   per eye e (0 left, 1 right), over the ommatidia i of omm[w][e][i][2]:
 *     dark_i = omm[i][0] + omm[i][1] < obj_threshold        (strict; one channel is always 0, so the sum is the reading)
 *     cnt = #dark, Sx = sum_dark qx_i, Sy = sum_dark qy_i   (int32; (qx_i, qy_i) = centres[i]: int16 sixteenths of a pixel)
 *     cy = Sy / (16 cnt height), cx = Sx / (16 cnt width), area = cnt / n_omm;  (1/2, 1/2, 0) when cnt = 0
 *       (each quotient: the correctly rounded float64 division of the exact integers, rounded once to float32)
 *     dev = front_edge[e] ? 1 - cx : cx                      (the object's distance from the image edge that faces forward)
 *     v_e = area > area_threshold ? min(max(1 - visual_gain dev, v_min), v_max) : 1
 *   over the odor dimensions d of odor[w][d][4] (sites: palp left, palp right, antenna left, antenna right):
 *     L_d = w_ant I[d][2] + w_palp I[d][0], R_d = w_ant I[d][3] + w_palp I[d][1], s_d = L_d + R_d
 *     c_d = s_d > 0 ? (L_d - R_d) / s_d : 0                 (correctly rounded)
 *   b = sum_d gains[d] c_d (ascending d, from 0);  q = (b |b|) / (1 + b b) (correctly rounded)
 *   o_0 = 1 - odor_delta max(q, 0), o_1 = 1 - odor_delta max(-q, 0)
 *   drive[side] = min(max((base v_side) o_side, drive_min), drive_max)          (side 0 = left: the order of NMF_CPG_DRIVE)
 * Everything after the features is float32 with every operation rounded as written (no contraction, no reassociation), so the
 * outputs equal the specification's bit for bit whatever the order of the integer reduction.  Without omm, v = 1 and the
 * features are (1/2, 1/2, 0); without odor, b = 0 and o = 1. */
typedef struct nmf_taxis_params {
  float obj_threshold;          /* a reading below this is dark                                                          */
  float area_threshold;         /* an eye has found an object when more than this share of its ommatidia is dark         */
  float visual_gain, v_min, v_max;
  float w_ant, w_palp;          /* weights of the antenna and the palp of a side                                         */
  float odor_delta;
  float base, drive_min, drive_max;
  int32_t front_edge[2];        /* per eye: 1 when the image's LAST column faces forward, 0 when column 0 does           */
} nmf_taxis_params;

/* sizeof(nmf_taxis_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_taxis_params_size(void);

/* One steering update of n_worlds worlds.  Device buffers: centres_dev[n_omm][2] int16 (4-byte aligned), omm_dev
 * [n_worlds][2][n_omm][2] float32 (8-byte aligned) or NULL, odor_dev[n_worlds][n_dims][4] float32 (16-byte aligned) or NULL,
 * odor_gains_dev[n_dims] float32; outputs features_dev[n_worlds][2][3] float32 (cy, cx, area per eye) or NULL, bias_dev[n_worlds]
 * float32 (b) or NULL, drive_dev[n_worlds][2] float32.  `params` is host memory, read during the call.  Argument checks and ONE
 * kernel launch on `stream` (of the calling thread's current device): no allocation, no host synchronisation, hipGraph-capturable.
 * Refused (nmf_last_error): null params or drive; omm and odor both null; n_worlds < 1; n_dims outside 0..8; with omm: n_omm
 * outside 1..1024, height or width outside 1..2047, null centres; with odor and n_dims > 0: null gains; a misaligned buffer. */
int nmf_taxis_update(const nmf_taxis_params* params, const int16_t* centres_dev, int n_omm, int height, int width,
                     const float* omm_dev, const float* odor_dev, const float* odor_gains_dev, int n_dims, int n_worlds,
                     float* features_dev, float* bias_dev, float* drive_dev, void* stream);

/* Path integration with its state on the device (flygym_amd.sensors.PathIntegrator; csrc/nmf_odometry.hip): the fly's heading and
 * position estimated from proprioception alone — how far each leg's tip travels backwards along the body's x axis while the leg is
 * on the ground.  No reference counterpart (the snapshot holds no path integration): build-defined and pinned by nothing, in the
 * form of flygym 1.x's path-integration task (specification tests/odometry_spec.py).
 * State per world: count (int32, updates since the reset); per leg (LEGS order lf lm lh rf rm rh) the last body-frame fore-aft
 * coordinate xprev (float32), the last contact flag cprev and the cumulative stride total (float64); a ring of the last `window`
 * totals (float64); the estimates heading (float64, radians, kept in [-pi, pi]) and position[2] (float64).  Shared by all worlds of
 * a handle, in device memory and writable between launches: 14 float64 coefficients in the order heading_coef[6], disp_coef[6],
 * heading_bias, disp_bias.  One update (one launch per control tick) reads the batch's seg_xpos, seg_xquat and sensordata as they
 * stand when it starts; every right-hand side is taken from the old state:
 *   xhat   = the root segment's x axis: (1 - 2 (qy qy + qz qz), 2 (qx qy + qw qz), 2 (qx qz - qw qy)) of its quaternion, float32
 *   x_l    = fl(fl(fl(dx ax) + fl(dy ay)) + fl(dz az)),  d = position of tip_seg[l] - position of root_seg        (float32)
 *   c_l    = found_l > 0 and (thr_l == 0 or fl(fl(fx^2 + fy^2) + fz^2) > fl(thr_l^2))      (sensor l's values 0..3; |F| does not
 *                                                                                            depend on the frame it is reported in)
 *   inc_l  = (count > 0 and c_l and cprev_l) ? (double) fl(xprev_l - x_l) : 0     (stance moves the tip backwards: positive when
 *                                                                                   walking forwards)
 *   total_l <- total_l + inc_l                                                                                    (float64)
 *   slot   = count mod window;  win_l = total_l(new) - ring[slot][l];  ring[slot][l] <- total_l(new)
 *   valid  = count >= window                                  (win then spans exactly `window` updates)
 *   dh = heading_bias + sum_{l = 0..5} heading_coef_l win_l,  dd = disp_bias + sum_l disp_coef_l win_l   (float64, ascending l)
 *   dh, dd <- dh inv_window, dd inv_window                    (inv_window = 1.0 / window, computed once on the host in float64)
 *   if valid: heading <- wrap(heading + dh),  wrap(h) = h - 2 pi rint(h (1 / 2 pi))    (the float64 constants 6.283185307179586
 *                                                                                        and 0.15915494309189535; also applied
 *                                                                                        to a reset's heading)
 *   (s, c) = sine and cosine of (float) heading(new) — the heading rounded to float32 —, evaluated in float64 (within 2e-15 of
 *            the exact ones: position and home stay within 1e-7 of the distance covered of a float64 evaluation of these lines)
 *   if valid: position <- position + dd (c, s)                                                                    (float64)
 *   home   = (-(c px + s py), -(-s px + c py)) of the new position: the way back to the estimate's origin in the body frame
 *   xprev_l <- x_l, cprev_l <- c_l, count <- count + 1
 * Every product, sum and difference above is rounded on its own (no contraction, no reassociation) and nothing is divided, so the
 * state equals the specification's bit for bit up to the sine and cosine.  The first update after a reset only primes xprev and
 * cprev; during the first `window` updates the estimates stand still (flygym 1.x likewise starts estimating after one window).
 * A pose that is not finite propagates into that world's state until the world is reset. */
typedef struct nmf_odometry_params {
  int32_t window;               /* updates a stride window spans (1..4096)                                               */
  int32_t root_seg;             /* index of the body's root segment in the batch's segment order                         */
  int32_t tip_seg[6];           /* per leg: the segment whose origin is the leg's tip                                    */
  float contact_force_threshold[6];   /* per leg: the leg is on the ground when |F| exceeds it (0: whenever found > 0)    */
} nmf_odometry_params;

/* sizeof(nmf_odometry_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_odometry_params_size(void);

/* An explicit handle for the worlds of `batch`, on its device.  coef_host: the 14 float64 coefficients in HOST memory, or NULL for
 * zeros.  Owns the state arrays and resets every world (nmf_odometry_reset with NULL mask and pose).  NOT stream-ordered
 * (allocations, synchronous uploads); must not be called inside a stream capture.  NULL on error (nmf_last_error), with nothing
 * left allocated: window outside 1..4096; root_seg or a tip_seg outside the batch's segments; a threshold that is negative or not
 * finite; a coefficient that is not finite; a batch whose model has no six leg sensors (as nmf_cpg_hybrid_enable); no device
 * memory.  The handle keeps pointers to the batch's seg_xpos / seg_xquat / sensordata arrays: destroy it before the batch. */
nmf_odometry* nmf_odometry_create(nmf_batch* batch, const nmf_odometry_params* params, const double* coef_host);
void nmf_odometry_destroy(nmf_odometry* odometry);

/* The worlds with mask_dev[w] != 0 (uint8 per world, device memory; NULL: all) get count = 0, totals, window strides and ring rows
 * 0, no previous sample (the next update primes again), and the estimate pose_dev[w] = (x, y, heading) (float64
 * [n_worlds][3], device memory; NULL: zeros) with the home vector that belongs to it; the others are not touched.  Stream-ordered. */
int nmf_odometry_reset(nmf_odometry* odometry, const uint8_t* mask_dev, const double* pose_dev, void* stream);

/* One update of every world: ONE kernel launch on `stream`, no allocation, no host synchronisation, hipGraph-capturable (count
 * lives on the device, so a captured update replays correctly any number of times). */
int nmf_odometry_update(nmf_odometry* odometry, void* stream);

/* Device pointer + row width of an array of the handle (zero-copy views; writable between launches). */
#define NMF_ODOMETRY_TOTAL 0      /* [6] float64: cumulative stride per leg                                   */
#define NMF_ODOMETRY_WINDOW 1     /* [6] float64: win of the last update                                      */
#define NMF_ODOMETRY_HEADING 2    /* [1] float64                                                              */
#define NMF_ODOMETRY_POSITION 3   /* [2] float64                                                              */
#define NMF_ODOMETRY_HOME 4       /* [2] float64                                                              */
#define NMF_ODOMETRY_COUNT 5      /* [1] int32                                                                */
#define NMF_ODOMETRY_COEF 6       /* ONE row of 14 float64 shared by all worlds (width 14; not per world)     */
void* nmf_odometry_field_ptr(nmf_odometry* odometry, int which, int32_t* width);

/* Motion vision with its state on the device (flygym_amd.sensors.MotionDetectors; csrc/nmf_motion.hip): how the image of each eye
 * moves, from correlating neighbouring ommatidia over time, and an optomotor drive that turns the fly with the panorama so that it
 * holds its course.  No reference counterpart (the snapshot holds no vision processing): build-defined and pinned by nothing
 * (specification tests/motion_spec.py).
 * Shared by all worlds of a handle: a list of n_pairs pairs (a_k, b_k, wx_k, wy_k) — two neighbouring ommatidia a != b and the
 * float32 unit vector from a to b in image coordinates (x = column, y = row).  State per world: a "fresh" byte and, per eye and
 * ommatidium, two float32 low-pass states fast and slow.  One update (one launch per control tick), per world:
 *   per eye e (0 left, 1 right), over the ommatidia i of omm[w][e][i][2]:
 *     x_i = omm[i][0] + omm[i][1]                            (one channel is always 0, so the sum is the reading)
 *     if the world is fresh: fast_i = slow_i = x_i
 *     fast_i <- fast_i + fl(a_fast fl(x_i - fast_i)),  slow_i <- slow_i + fl(a_slow fl(x_i - slow_i)),  hp_i = x_i - slow_i(new)
 *   per eye, over the pairs k, with the values just computed (a Hassenstein-Reichardt correlator per pair):
 *     d_k = fl(fast_a hp_b) - fl(hp_a fast_b)
 *     Sx += (int32) rint(min(max(fl(d_k wx_k), -4), 4) 65536),  Sy likewise with wy_k
 *       (terms of resolution 2^-16 clamped to +-4, a NaN counting as -4: with n_pairs <= 3072 a sum stays below 2^30 for any
 *        readings, and integer sums do not depend on the order of the reduction)
 *     H_e = Sx / (65536 n_pairs), V_e = Sy / (65536 n_pairs)  (each: the correctly rounded float64 division of the exact
 *                                                              operands, rounded once to float32); 0 when n_pairs = 0
 *   ftb_e = front_edge[e] ? -H_e : H_e                       (the flow from front to back across eye e)
 *   rotation = ftb_0 - ftb_1     (positive when the panorama turns counter-clockwise about the fly, seen from above)
 *   translation = ftb_0 + ftb_1                              (a zero of either is +0)
 *   r = gain rotation;  q = r / (1 + |r|) (correctly rounded as above);  o_0 = 1 - delta max(q, 0), o_1 = 1 - delta max(-q, 0)
 *   drive[side] = min(max(base[side] o_side, drive_min), drive_max)      (side 0 = left: the order of NMF_CPG_DRIVE; base[side]
 *                                                                         from base_dev, or the parameter `base` without it)
 *   the world is no longer fresh
 * So a counter-clockwise panorama slows the left side and the fly turns with it.  Every float32 operation is rounded as written
 * (no contraction, no reassociation): state and outputs equal the specification's bit for bit.  a_fast and a_slow are
 * 1 - exp(-dt / tau) of the caller's control tick dt, computed in float64 on the host and rounded once to float32. */
typedef struct nmf_motion_params {
  float a_fast, a_slow;         /* low-pass coefficients of the two filters (defaults: tau 35 ms and 150 ms)              */
  float gain, delta;            /* optomotor rule: r = gain rotation; a side is slowed by at most delta                    */
  float base, drive_min, drive_max;
  int32_t front_edge[2];        /* per eye: 1 when the image's LAST column faces forward, 0 when column 0 does             */
} nmf_motion_params;

/* sizeof(nmf_motion_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_motion_params_size(void);

/* An explicit handle for the worlds of `batch`, on its device.  pairs_host[n_pairs][2] int32 and weights_host[n_pairs][2] float32
 * are HOST memory (either may be NULL when n_pairs is 0), copied.  Owns the pair list, the state and the outputs; every world
 * starts fresh.  NOT stream-ordered (allocations, synchronous uploads); must not be called inside a stream capture.  NULL on error
 * (nmf_last_error), with nothing left allocated: n_omm outside 1..1024; n_pairs outside 0..3072; a pair index outside 0..n_omm-1;
 * a pair with a == b; a weight or a parameter that is not finite; a_fast or a_slow outside [0, 1]; no device memory. */
nmf_motion* nmf_motion_create(nmf_batch* batch, const nmf_motion_params* params, const int32_t* pairs_host,
                              const float* weights_host, int n_pairs, int n_omm);
void nmf_motion_destroy(nmf_motion* motion);

/* The worlds with mask_dev[w] != 0 (uint8 per world, device memory; NULL: all) become fresh: their next update starts both
 * filters from its readings, exactly as a first update does.  The others are not touched.  Stream-ordered. */
int nmf_motion_reset(nmf_motion* motion, const uint8_t* mask_dev, void* stream);

/* One update of every world from omm_dev[n_worlds][2][n_omm][2] float32 (8-byte aligned): argument checks and ONE kernel launch on
 * `stream`, no allocation, no host synchronisation, hipGraph-capturable (the fresh bytes live on the device, so a captured update
 * replays correctly).  base_dev[n_worlds][2] float32 or NULL (the parameter `base`); the drive goes to drive_out_dev[n_worlds][2]
 * float32 (for example NMF_CPG_DRIVE, or the handle's own NMF_MOTION_DRIVE).  Refused: a null handle, omm or drive; a misaligned
 * buffer. */
int nmf_motion_update(nmf_motion* motion, const float* omm_dev, const float* base_dev, float* drive_out_dev, void* stream);

/* Device pointer + row width of an array of the handle (zero-copy views; writable between launches). */
#define NMF_MOTION_FAST 0         /* [2][n_omm] float32                                                        */
#define NMF_MOTION_SLOW 1         /* [2][n_omm] float32                                                        */
#define NMF_MOTION_SUMS 2         /* [2][2] int32: Sx, Sy per eye                                              */
#define NMF_MOTION_FLOW 3         /* [2][2] float32: H, V per eye                                              */
#define NMF_MOTION_ROTATION 4     /* [1] float32                                                               */
#define NMF_MOTION_TRANSLATION 5  /* [1] float32                                                               */
#define NMF_MOTION_DRIVE 6        /* [2] float32: a drive buffer of the handle's own (starts at 1)             */
#define NMF_MOTION_FRESH 7        /* [1] uint8                                                                 */
void* nmf_motion_field_ptr(nmf_motion* motion, int which, int32_t* width);

/* A retinotopic visual network with its state on the device (flygym_amd.sensors.RetinotopicNetwork; csrc/nmf_visnet.hip): cell
 * types that are layers of one cell per ommatidium, joined by small convolution kernels on the hexagonal lattice of the retina and
 * integrated as a leaky recurrent system, in the manner of Lappalainen et al. 2024 as flygym 1.x's "advanced vision" task reads it;
 * the pooled activity of the types, not the image, drives the CPG.  No reference counterpart (the snapshot holds no vision
 * processing): build-defined and pinned by nothing (specification tests/visnet_spec.py).
 * Shared by all worlds of a handle: C cell types, per type c the float32 constants bias_c, in_w[c][0..1], a_c, steer_w_c; a
 * neighbour table neighbours[2][T][n_omm] int32 per eye (row t: the ommatidium that lies at lattice offset t from ommatidium i, or
 * -1; see Retina.hex_neighbours; the two eyes' tables differ where the caller mirrors one eye's lattice so that an offset means
 * the same direction about the fly in both); E edges (post, pre) between types; and a flat tap list, tap k = (edge, t, w) with t a row of the table.
 * State per world and eye: a "fresh" byte and v[c][i] float32, one cell per type and ommatidium.  One update (at most two launches
 * per control tick), per world and eye e (0 left, 1 right), from omm[w][e][i][2]:
 *   x0_i = omm[i][0], x1_i = omm[i][1];  if the eye is fresh: v[c][i] = bias_c
 *   `substeps` times, every type from the OLD state of every type (synchronous):
 *     r[c][i] = v[c][i] > 0 ? v[c][i] : +0
 *     s = bias_c;  s = fmaf(in_w[c][0], x0_i, s);  s = fmaf(in_w[c][1], x1_i, s)
 *     for the edges into c in the caller's order, for the taps of each edge in the caller's order:
 *       j = neighbours[e][t][i];  s = fmaf(w, j >= 0 ? r[pre][j] : +0, s)     (a missing neighbour still executes its fmaf)
 *     v[c][i] <- v[c][i] + fl(a_c fl(s - v[c][i]))
 *   S[c] = sum_i (int32) rint(min(r[c][i], 4) 65536) of the NEW state
 *       (terms of resolution 2^-16 in [0, 4]: with n_omm <= 1024 a sum stays below 2^29, and integer sums do not depend on the
 *        order of the reduction)
 *   pooled[c] = S[c] / (65536 n_omm)       (the correctly rounded float64 division of the exact operands, rounded once to float32)
 *   the eye is no longer fresh
 * and per world:
 *   t = +0;  for c ascending: t = fmaf(steer_w_c, fl(pooled[0][c] - pooled[1][c]), t)          (a zero is +0: the signal)
 *   g = gain t;  q = g / (1 + |g|) (correctly rounded as above);  o_0 = 1 - delta max(q, 0), o_1 = 1 - delta max(-q, 0)
 *   drive[side] = min(max(base[side] o_side, drive_min), drive_max)      (side 0 = left: the order of NMF_CPG_DRIVE; base[side]
 *                                                                         from base_dev, or the parameter `base` without it)
 * Every float32 operation is rounded as written (no contraction, no reassociation, an fmaf where one is written): state and outputs
 * equal the specification's bit for bit.  a_c is 1 - exp(-dt / (substeps tau_c)) of the caller's control tick dt, computed in
 * float64 on the host and rounded once to float32. */
#define NMF_VISNET_MAX_TYPES 32       /* C                                                      */
#define NMF_VISNET_MAX_CELLS 24576    /* C x n_omm: 96 KiB of state, held in one CU's LDS       */
#define NMF_VISNET_MAX_TABLE 19       /* T: the lattice points within two pitches               */
#define NMF_VISNET_MAX_EDGES 512      /* E                                                      */
#define NMF_VISNET_MAX_TAPS 4096      /* taps of all edges together                             */
#define NMF_VISNET_MAX_SUBSTEPS 8
typedef struct nmf_visnet_params {
  int32_t n_types, n_omm, n_table, n_edges, n_taps;      /* C, ommatidia per eye, T, E, taps in all                        */
  int32_t substeps;                                      /* 1..8 repetitions of the rule per update                        */
  float gain, delta;                                     /* optomotor rule: g = gain t; a side is slowed by at most delta  */
  float base, drive_min, drive_max;
} nmf_visnet_params;

/* sizeof(nmf_visnet_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_visnet_params_size(void);

/* An explicit handle for the worlds of `batch`, on its device.  HOST memory, copied: types_host[C][5] float32 (bias, in_w[0],
 * in_w[1], a, steer_w per type), neighbours_host[2][T][n_omm] int32, edges_host[E][2] int32 (post, pre), taps_host[n_taps][2] int32
 * (edge, t) and tap_w_host[n_taps] float32 (the last three may be NULL when their count is 0).  Owns the network, the state and the
 * outputs; every world starts fresh.  NOT stream-ordered (allocations, synchronous uploads); must not be called inside a stream
 * capture.  NULL on error (nmf_last_error names the offending entry), with nothing left allocated: n_types outside 1..32; n_omm
 * outside 1..1024; n_types x n_omm above 24576; n_table outside 1..19; n_edges outside 0..512; n_taps outside 0..4096; substeps
 * outside 1..8; a constant, weight or parameter that is not finite; a_c outside (0, 1]; a neighbour outside -1..n_omm-1; an edge
 * whose types lie outside 0..C-1; a tap whose edge lies outside 0..E-1 or whose t lies outside 0..T-1; no device memory. */
nmf_visnet* nmf_visnet_create(nmf_batch* batch, const nmf_visnet_params* params, const float* types_host,
                              const int32_t* neighbours_host, const int32_t* edges_host, const int32_t* taps_host,
                              const float* tap_w_host);
void nmf_visnet_destroy(nmf_visnet* visnet);

/* Both eyes of the worlds with mask_dev[w] != 0 (uint8 per world, device memory; NULL: all) become fresh: their next update
 * starts from v[c][i] = bias_c, exactly as a first update does.  The others are not touched.  Stream-ordered. */
int nmf_visnet_reset(nmf_visnet* visnet, const uint8_t* mask_dev, void* stream);

/* One update of every world from omm_dev[n_worlds][2][n_omm][2] float32 (8-byte aligned): argument checks and TWO kernel launches
 * on `stream` (the network per world and eye, then signal and drive per world), no allocation, no host synchronisation,
 * hipGraph-capturable (the fresh bytes live on the device, so a captured update replays correctly).  base_dev[n_worlds][2] float32
 * or NULL (the parameter `base`); the drive goes to drive_out_dev[n_worlds][2] float32 (for example NMF_CPG_DRIVE, or the
 * handle's own NMF_VISNET_DRIVE).  Refused: a null handle, omm or drive; a misaligned buffer. */
int nmf_visnet_update(nmf_visnet* visnet, const float* omm_dev, const float* base_dev, float* drive_out_dev, void* stream);

/* Device pointer + row width of an array of the handle (zero-copy views; writable between launches). */
#define NMF_VISNET_V 0            /* [2][C][n_omm] float32                                                     */
#define NMF_VISNET_POOLED 1       /* [2][C] float32                                                            */
#define NMF_VISNET_SUMS 2         /* [2][C] int32                                                              */
#define NMF_VISNET_SIGNAL 3       /* [1] float32                                                               */
#define NMF_VISNET_DRIVE 4        /* [2] float32: a drive buffer of the handle's own (starts at 1)             */
#define NMF_VISNET_FRESH 5        /* [2] uint8                                                                 */
void* nmf_visnet_field_ptr(nmf_visnet* visnet, int which, int32_t* width);

/* Plume navigation with its state on the device (flygym_amd.controllers.PlumeNavigator; csrc/nmf_navigator.hip): a stochastic walk /
 * stop / turn state machine driven by odor onsets ("encounters"), in the form of Demir et al. 2020 as flygym 1.x steered its
 * plume-tracking task with it.  No reference counterpart (the snapshot holds no controllers): build-defined and pinned by nothing
 * (specification tests/navigator_spec.py).
 * State per world: state (int32: the NMF_NAV_ values below), remaining (int32, ticks left of a turn), above (uint8: the antennal sum
 * was above the threshold in the last update), the leaky filters k_stop, k_walk and freq (float32), ticks (uint32, updates since
 * the reset: the noise counter), encounters (int32, cumulative) and drive[2] (float32: left, right, the order of NMF_CPG_DRIVE).
 * One update (one launch per control tick) reads odor[w][odor_dim][4] (palp L, palp R, antenna L, antenna R: the layout of
 * nmf_odor_intensity and nmf_plume_sample_sites), the wind (wx, wy) of row w or of the one shared row, and the quaternion
 * (qw, qx, qy, qz) of root_seg in the batch's seg_xquat as it stands.  Everything is float32, every operation is rounded on its own
 * (no contraction, no reassociation), and every right-hand side is the old state except that the probabilities use the filters
 * just updated:
 *   s = I[2] + I[3];  now = s > threshold (false for a NaN);  e = now and not above;  above <- now;  encounters <- encounters + e
 *   k_stop <- fl(k_stop decay_stop) + e;  k_walk <- fl(k_walk decay_walk) + e;  freq <- fl(freq decay_freq) + (e ? inv_tau_freq : 0)
 *   ax = 1 - 2 (qy qy + qz qz),  ay = 2 (qx qy + qw qz)          (the body's x axis in the ground plane, as nmf_odometry_update)
 *   cross = fl(ay wx) - fl(ax wy)                                (> 0: upwind, the direction -wind, lies to the left; false for a NaN)
 *   u_m = (hash(seed ^ (first_world + w) 0x9E3779B9 ^ ticks 0x85EBCA6B ^ (8 + m) 0xC2B2AE35) >> 8) 2^-24,  m = 0, 1, 2
 *         (uint32 arithmetic; the mixer and the key of csrc/nmf_plume.hip, whose wind noise uses the draw indices 0..7)
 *   c01(x) = x < 0 ? 0 : (x > 1 ? 1 : x)                         (comparisons: a NaN would pass through)
 *   p_stop = c01(dt (lambda_ws0 + dlambda_ws k_stop)),  p_walk = c01(dt (lambda_sw0 + dlambda_sw k_walk)),  p_turn = c01(dt lambda_turn)
 *   x = p_up0 + up_gain freq;  p_up = x < p_up_min ? p_up_min : (x > p_up_max ? p_up_max : x)
 *   a turn (state TURN_LEFT or TURN_RIGHT): remaining <- remaining - 1; when that is <= 0 the state becomes WALK
 *   WALK: u_0 < p_stop -> STOP;  else u_1 < p_turn -> remaining <- turn_ticks and a turn towards (u_2 < p_up ? upwind : downwind):
 *         TURN_LEFT when (towards upwind) == (cross > 0), else TURN_RIGHT
 *   STOP: u_0 < p_walk -> WALK
 *   ticks <- ticks + 1;  drive <- the row of the NEW state: walk_drive, stop_drive, turn_drive = (inner, outer) with the inner side
 *         left for TURN_LEFT, swapped for TURN_RIGHT
 * So a turn holds its drive row for exactly turn_ticks updates.  Nothing is divided and no function is called: decay_x =
 * exp(-dt / tau_x) and inv_tau_freq = 1 / tau_freq come from the caller, computed in float64 and rounded once to float32, and
 * turn_ticks = round(turn_duration / dt).  Readings, winds and attitudes that are not finite only ever reach comparisons: the state
 * stays finite.  A world's noise depends on (seed, first_world + w, ticks) alone: not on the batch it is stepped in. */
#define NMF_NAV_WALK 0
#define NMF_NAV_STOP 1
#define NMF_NAV_TURN_LEFT 2
#define NMF_NAV_TURN_RIGHT 3
typedef struct nmf_navigator_params {
  uint32_t seed;                /* of the noise streams                                                                   */
  int32_t first_world;          /* global index of world 0 (a shard of a larger population); >= 0                         */
  int32_t root_seg;             /* index of the body's root segment in the batch's segment order                          */
  int32_t odor_dim;             /* the odor dimension whose antennae are read (0..7)                                      */
  int32_t turn_ticks;           /* updates a turn lasts (1..65535)                                                        */
  float dt;                     /* the control tick in seconds: rates become probabilities per update                     */
  float threshold;              /* of the antennal sum (>= 0)                                                             */
  float decay_stop, decay_walk, decay_freq;   /* per update, each in [0, 1]                                              */
  float inv_tau_freq;           /* what an encounter adds to freq                                                         */
  float lambda_ws0, dlambda_ws; /* walk -> stop rate per second: the base and its change per unit of k_stop               */
  float lambda_sw0, dlambda_sw; /* stop -> walk rate likewise, per unit of k_walk                                         */
  float lambda_turn;            /* turn rate per second while walking                                                     */
  float p_up0, up_gain, p_up_min, p_up_max;   /* the probability that a turn goes upwind: bounds in [0, 1], min <= max   */
  float walk_drive[2], stop_drive[2];         /* (left, right)                                                           */
  float turn_drive[2];          /* (inner, outer)                                                                         */
} nmf_navigator_params;

/* sizeof(nmf_navigator_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_navigator_params_size(void);

/* An explicit handle for the worlds of `batch`, on its device.  Owns the state arrays and resets every world (nmf_navigator_reset
 * with a NULL mask).  NOT stream-ordered (allocations); must not be called inside a stream capture.  NULL on error
 * (nmf_last_error), with nothing left allocated: a parameter that is not finite; a threshold below 0; a decay outside [0, 1];
 * p_up_min > p_up_max or either outside [0, 1]; turn_ticks outside 1..65535; root_seg outside the batch's segments; odor_dim
 * outside 0..7; first_world below 0; no device memory.  The handle keeps a pointer to the batch's seg_xquat array: destroy it
 * before the batch. */
nmf_navigator* nmf_navigator_create(nmf_batch* batch, const nmf_navigator_params* params);
void nmf_navigator_destroy(nmf_navigator* navigator);

/* The worlds with mask_dev[w] != 0 (uint8 per world, device memory; NULL: all) get state WALK, remaining 0, above 0, empty
 * filters, ticks 0 (their noise stream starts again), encounters 0 and walk_drive in the handle's own drive array; the others are
 * not touched.  Stream-ordered. */
int nmf_navigator_reset(nmf_navigator* navigator, const uint8_t* mask_dev, void* stream);

/* One update of every world from odor_dev[n_worlds][n_dims][4] float32 (16-byte aligned) and wind_dev[wind_rows][2] float32
 * (wind_rows = n_worlds, or 1: one row shared by all worlds): argument checks and ONE kernel launch on `stream`, no allocation, no
 * host synchronisation, hipGraph-capturable (ticks lives on the device, so a captured update draws fresh noise on every replay).
 * The drive goes to drive_out_dev[n_worlds][2] float32 (8-byte aligned; for example NMF_CPG_DRIVE) or, when that is NULL, to the
 * handle's own NMF_NAVIGATOR_DRIVE.  Refused: a null handle, odor or wind; n_dims <= odor_dim; wind_rows neither 1 nor n_worlds;
 * a misaligned buffer. */
int nmf_navigator_update(nmf_navigator* navigator, const float* odor_dev, int n_dims, const float* wind_dev, int wind_rows,
                         float* drive_out_dev, void* stream);

/* Device pointer + row width of an array of the handle (zero-copy views; writable between launches). */
#define NMF_NAVIGATOR_STATE 0       /* [1] int32                                                               */
#define NMF_NAVIGATOR_REMAINING 1   /* [1] int32                                                               */
#define NMF_NAVIGATOR_ABOVE 2       /* [1] uint8                                                               */
#define NMF_NAVIGATOR_K_STOP 3      /* [1] float32                                                             */
#define NMF_NAVIGATOR_K_WALK 4      /* [1] float32                                                             */
#define NMF_NAVIGATOR_FREQ 5        /* [1] float32                                                             */
#define NMF_NAVIGATOR_TICKS 6       /* [1] uint32                                                              */
#define NMF_NAVIGATOR_ENCOUNTERS 7  /* [1] int32                                                               */
#define NMF_NAVIGATOR_DRIVE 8       /* [2] float32: the drive buffer of the handle's own (starts at walk_drive)*/
void* nmf_navigator_field_ptr(nmf_navigator* navigator, int which, int32_t* width);

/* Head stabilization: a small network drives the neck (flygym_amd.controllers.HeadStabilizer; csrc/nmf_stabilizer.hip), in the form
 * of flygym 1.x's head-stabilization model: an MLP from the leg joint angles and the leg contact flags to the neck's roll and pitch
 * that cancel the thorax's rocking.  No reference counterpart (the snapshot holds no controllers): build-defined and pinned by
 * nothing (specification tests/stabilizer_spec.py).  The primitive is a per-world MLP evaluated in one launch.
 * Stateless.  One update (one launch per control tick) reads the batch's qpos and sensordata as they stand and, per world w, in
 * float32:
 *   x[k]       = fl(fl(qpos[w][7 + dof[k]] - mean[k]) inv_std[k])                 k < n_q   (two roundings; nothing is divided)
 *   m_l        = fmaf(Fz, Fz, fmaf(Fy, Fy, fl(Fx Fx)))                            F = sensordata[w][16 l + 1 .. 3], leg l's net force
 *   x[n_q + l] = (sensordata[w][16 l] > 0 and m_l > thr2[l]) ? 1 : 0              l < 6, when contacts != 0: n_in = n_q + 6, else n_q
 *   h_0 = x;  layer i = 0 .. n_hidden:  a[j] = b_i[j];  for k ascending: a[j] = fmaf(W_i[j][k], h_{i-1}[k], a[j])
 *             a hidden layer: h_i[j] = a[j] > 0 ? a[j] : 0;   the last layer: y[j] = a[j]
 *   y[j]       = y[j] < lo[j] ? lo[j] : (y[j] > hi[j] ? hi[j] : y[j])             (comparisons)
 *   out[w][j]  = y[j];  and, when the handle has actuator ids:  ctrl[w][act[j]] = y[j]
 * fmaf is the fused multiply-add: one rounding per step of a chain that starts at the bias and runs over the inputs in ascending
 * order.  That order is the specification; how the work is split over lanes is not.  thr2 is the squared force threshold, mean
 * and inv_std = 1 / std come from the caller.  Values of qpos and sensordata that are not finite are outside the contract: they
 * index nothing, and nothing is said about the results' bits. */
#define NMF_STABILIZER_MAX_HIDDEN 3      /* hidden layers                                    */
#define NMF_STABILIZER_MAX_WIDTH 64      /* units of a hidden layer                          */
#define NMF_STABILIZER_MAX_IN 256        /* n_in                                             */
#define NMF_STABILIZER_MAX_OUT 8         /* n_out                                            */
typedef struct nmf_stabilizer_params {
  int32_t n_q;                  /* joint angles read (>= 1)                                                               */
  int32_t contacts;             /* != 0: the six contact flags follow the joint angles                                    */
  int32_t n_hidden;             /* hidden layers (1..3)                                                                   */
  int32_t hidden[3];            /* their widths (1..64 each); entries past n_hidden are ignored                           */
  int32_t n_out;                /* outputs (1..8)                                                                         */
  float thr2[6];                /* squared contact-force threshold per leg (legs in LEGS order); read when contacts != 0  */
  float lo[8], hi[8];           /* the outputs' bounds, lo[j] <= hi[j]; entries past n_out are ignored                    */
} nmf_stabilizer_params;

/* sizeof(nmf_stabilizer_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_stabilizer_params_size(void);

/* An explicit handle for the worlds of `batch`, on its device.  Host arrays, copied: dof[n_q] int32 (joint dof indices: qpos
 * column 7 + dof[k]; repeats are allowed), mean[n_q] and inv_std[n_q] float32, `weights` float32 = W_0 (row-major
 * [hidden[0]][n_in]), b_0, W_1, b_1, ... up to the output layer's W ([n_out][width of the last hidden layer]) and b, and
 * act[n_out] int32 (control ids that receive the outputs) or NULL (the update only fills `out`).  Owns the uploaded network and
 * the (n_worlds, n_out) output array.  NOT stream-ordered (allocations); must not be called inside a stream capture.  NULL on error
 * (nmf_last_error), with nothing left allocated: n_hidden outside 1..3; a hidden width outside 1..64; n_q < 1; n_in > 256;
 * n_out outside 1..8; a dof[k] outside the model's joint dofs (0 .. nq - 8); an act[j] outside 0 .. nu - 1; lo[j] > hi[j]; a
 * weight, bias, mean, inv_std, thr2 or bound that is not finite; contacts on a batch whose sensordata is not six leg sensors of 16
 * values; a null batch, params, dof, mean, inv_std or weights; no device memory.  The handle keeps pointers to the batch's qpos,
 * sensordata and ctrl arrays: destroy it before the batch. */
nmf_stabilizer* nmf_stabilizer_create(nmf_batch* batch, const nmf_stabilizer_params* params, const int32_t* dof, const float* mean,
                                      const float* inv_std, const float* weights, const int32_t* act);
void nmf_stabilizer_destroy(nmf_stabilizer* stabilizer);

/* One update of every world: argument checks and ONE kernel launch on `stream`, no allocation, no host synchronisation,
 * hipGraph-capturable.  The outputs go to out_dev[n_worlds][n_out] float32 (16-byte aligned) or, when that is NULL, to the
 * handle's own NMF_STABILIZER_OUTPUT; with actuator ids they also go into the batch's ctrl.  No other device memory is written.
 * Refused: a null handle; a misaligned out_dev. */
int nmf_stabilizer_update(nmf_stabilizer* stabilizer, float* out_dev, void* stream);

/* Device pointer + row width of an array of the handle (zero-copy view; writable between launches). */
#define NMF_STABILIZER_OUTPUT 0     /* [n_out] float32: the output array of the handle's own (starts at 0)     */
void* nmf_stabilizer_field_ptr(nmf_stabilizer* stabilizer, int which, int32_t* width);

/* Rule-based walking with its state on the device (flygym_amd.controllers.RuleBasedController; csrc/nmf_rules.hip): legs start
 * steps by Cruse's rules 1 to 3, in the form of flygym 1.x's decentralised rule-based controller.  No reference counterpart (the
 * snapshot holds no controllers): build-defined and pinned by nothing (specification tests/rules_spec.py).
 * Tripod, tetrapod and wave gaits are not programmed: they follow from the weights.
 * Legs in LEGS order lf lm lh rf rm rh, side = leg / 3.  State per (world, leg): the counter k (int32, 0 <= k < P: 0 rests, a step
 * runs the leg's cycle once in P physics steps, swing first), stepping (uint8) and the latched amplitude a (float32).  State per
 * world: drive[2] (float32: left, right, the order of NMF_CPG_DRIVE) and the tick word (uint32, physics steps since the reset: the
 * noise counter).  Shared: P = period_steps; cycle[n_bins][n_pos] and leg_of_col[n_pos] as nmf_cpg_create takes them; per leg
 * start_bin[l], the bin its swing starts at, and swing_steps[l], the physics steps its swing lasts (1 .. P - 1); three weight
 * matrices W1, W2, W3 [src][tgt]; margin; max_amplitude.
 * One physics step of one world.  The drive is read once when the launch starts.  All float arithmetic is float32, every operation
 * rounded once as written (no contraction, no reassociation), clamps are comparisons.
 *   1. the row, from the state before the update, for leg l:
 *        x = (double)(k n_bins) / (double)P  (one correctly rounded float64 division),  i0 = floor(x),  f = (float)(x - i0)
 *        b0 = (start_bin[l] + i0) mod n_bins,  b1 = (b0 + 1) mod n_bins
 *        c = fl(fl(1 - f) cycle[b0][col]) + fl(f cycle[b1][col]),  rest = cycle[start_bin[l]][col]
 *        row[col] = rest + fl(a fl(c - rest))                         (a resting leg holds rest exactly, whatever a is)
 *        row[n_pos + l] = adhesion_off while 0 < k < swing_steps[l], else adhesion_on      (with the six adhesion columns)
 *   2. the scores, a pure function of the six counters:
 *        swinging_s = 0 < k_s < swing_steps[s]
 *        p_s = (float)max(0, k_s - swing_steps[s]) / (float)(P - swing_steps[s])           (correctly rounded)
 *        for target t, sources s ascending, each sum from 0:  r1 = sum (swinging_s ? W1[s][t] : 0)
 *        r2 = sum over p_s > 0 of fl(W2[s][t] fl(1 - p_s)),  r3 = sum over p_s > 0 of fl(W3[s][t] p_s),  score_t = (r1 + r2) + r3
 *   3. eligibility:  m = max_t score_t;  x = m - fl(|m| margin);  thr = x > 0 ? x : 0
 *        eligible_t = score_t >= thr and score_t > 0 and not stepping_t and drive[side_t] != 0
 *        the fallback: if no leg of the world is stepping and none is eligible, every leg with drive[side_t] != 0 is eligible
 *        (this starts the walk after a reset and starts it again after a stop)
 *   4. selection, n = the number of eligible legs, if n > 0:
 *        u = hash(seed ^ (first_world + w) 0x9E3779B9 ^ tick 0x85EBCA6B ^ NMF_RULES_DRAW 0xC2B2AE35)      (uint32 arithmetic: the
 *        mixer and the key of csrc/nmf_plume.hip, whose wind noise uses the draw indices 0..7 and the navigator 8..10)
 *        j = ((uint64)u n) >> 32;  the j-th eligible leg in ascending order gets stepping = 1 and
 *        a = |drive[side]| > max_amplitude ? max_amplitude : |drive[side]|               (the sign of a drive is ignored)
 *   5. advance: stepping legs k <- k + 1; at k = P: k <- 0, stepping <- 0
 *   6. tick <- tick + 1
 * scores keeps score_t of the last step.  A world's result depends on (seed, first_world + w, its state and its drive) alone: not on
 * the batch it is stepped in. */
#define NMF_RULES_DRAW 11            /* the draw index of the selection */
typedef struct nmf_rules_params {
  int32_t n_pos;                /* position-target columns of a row (1..4096)                                            */
  int32_t n_bins;               /* phase bins of the step cycle (2..2^20)                                                */
  int32_t period_steps;         /* P: physics steps of one step of a leg (>= 2, P n_bins < 2^31)                         */
  int32_t table_steps;          /* rows per world of the tables nmf_rules_advance will be given (>= 1)                   */
  int32_t adhesion;             /* != 0: six adhesion columns follow the position columns                                */
  float adhesion_on, adhesion_off;   /* their values out of swing / in swing                                            */
  float margin;                 /* relative distance from the best score within which a leg is eligible (>= 0)           */
  float max_amplitude;          /* the cap of the latched amplitude (>= 0)                                               */
  uint32_t seed;                /* of the selection's draws                                                              */
  int32_t first_world;          /* global index of world 0 (a shard of a larger population); >= 0                        */
} nmf_rules_params;

/* sizeof(nmf_rules_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_rules_params_size(void);

/* An explicit handle for the worlds of `batch`, on its device: takes HOST arrays — cycle[n_bins][n_pos] float32, leg_of_col[n_pos]
 * (each in 0..5), start_bin[6] (each in 0 .. n_bins - 1), swing_steps[6] (each in 1 .. P - 1), weights[3][6][6] float32 (W1, W2, W3
 * as [src][tgt]) — validates them, owns device copies and the state arrays, and resets every world (nmf_rules_reset with a NULL
 * mask).  NOT stream-ordered (allocations, synchronous uploads); must not be called inside a stream capture.  NULL on error
 * (nmf_last_error), with nothing left allocated: a size outside the ranges above; P n_bins >= 2^31; a leg_of_col, start_bin or
 * swing_steps outside its range; a weight, margin, max_amplitude or adhesion value that is not finite; a negative margin,
 * max_amplitude or first_world; a null argument; no device memory. */
nmf_rules* nmf_rules_create(nmf_batch* batch, const nmf_rules_params* params, const float* cycle, const int32_t* leg_of_col,
                            const int32_t* start_bin, const int32_t* swing_steps, const float* weights);
void nmf_rules_destroy(nmf_rules* rules);

/* The worlds with mask_dev[w] != 0 (uint8 per world, device memory; NULL: all) get k = 0, stepping = 0, a = 1, drive = (1, 1),
 * tick = 0 (their draws start again) and scores = 0; the others are not touched.  Stream-ordered. */
int nmf_rules_reset(nmf_rules* rules, const uint8_t* mask_dev, void* stream);

/* Device pointer + row width of a per-world array of the controller (zero-copy views; writable between launches).  A counter
 * written outside [0, P) is reduced modulo P by the next launch. */
#define NMF_RULES_COUNTER 0       /* [6] int32                     */
#define NMF_RULES_STEPPING 1      /* [6] uint8                     */
#define NMF_RULES_AMPLITUDE 2     /* [6] float32                   */
#define NMF_RULES_DRIVE 3         /* [2] float32 (left, right)     */
#define NMF_RULES_TICKS 4         /* [1] uint32                    */
#define NMF_RULES_SCORES 5        /* [6] float32                   */
void* nmf_rules_field_ptr(nmf_rules* rules, int which, int32_t* width);

/* Advance every world by n_steps and write table_dev[w][s][0 .. n_act) for s < n_steps (float32 [n_worlds][table_steps][n_act],
 * n_act = n_pos or n_pos + 6: the table of nmf_step_replay / nmf_step_record with start = 0); rows n_steps .. table_steps - 1 are
 * not touched.  Argument checks and ONE kernel launch on `stream`: no allocation, no host synchronisation, hipGraph-capturable
 * (the counters and the tick words live on the device, so a captured launch continues and draws afresh on every replay).
 * Refused: what nmf_cpg_advance refuses. */
int nmf_rules_advance(nmf_rules* rules, int n_steps, float* table_dev, int table_steps, void* stream);

/* The walking task on the device (flygym_amd.tasks.WalkingTask; csrc/nmf_task.hip): what an episode is, when it ends, what a tick
 * was worth and which worlds start again -- the layer flygym 1.x's Gymnasium environments (`step` -> obs, reward, terminated,
 * truncated, info, with flip detection) put around a walking fly.  No reference counterpart (the snapshot holds no tasks):
 * build-defined and pinned by nothing, and nothing is claimed about matching flygym 1.x (specification
 * tests/task_spec.py).  One update (one launch per control tick) reads, as they stand when the launch starts,
 *   from the batch:  (x, y, z) = seg_xpos[root_seg], (qw, qx, qy, qz) = seg_xquat[root_seg];  qvel[0:3] = (vx, vy, vz), the root's
 *     linear velocity in the WORLD frame, and qvel[3:6] = (ox, oy, oz), its angular velocity in the BODY frame (MuJoCo's free joint:
 *     the step integrates position += h qvel[0:3] and quat <- quat * exp(h qvel[3:6] / 2));  f_a = actuator_force[act[a]] and
 *     qd_a = qvel[6 + act_dof[a]], a < n_act;  of sensordata, per leg l the four floats (found, Fx, Fy, Fz) at [16 l .. 16 l + 3];
 *     ang_k = qpos[7 + obs_dof[k]], k < n_q
 *   from the handle:  course[w] = (cx, cy), a unit direction the host normalised, and goal[w] = (gx, gy)
 * and, per world, does the following.  Everything is float32, every operation is rounded on its own (no contraction, no
 * reassociation; fl() marks a rounding that matters), every clamp and every test is a comparison (false for a NaN), every stored
 * float that is a zero is +0, the counters are int32 that wrap, and `old` state is the state before the update.
 *   1. bad = one of the values just listed has all exponent bits set (NaN, +Inf, -Inf; tested on the bits).  A bad world gets
 *      reason = NONFINITE alone, reward = -penalty_fail exactly and an observation row of zeros; steps 2 to 6 decide nothing for it.
 *   2. progress = fresh ? 0 : fl(fl(fl(x - px) cx) + fl(fl(y - py) cy)),  (px, py) = prev_xy: the root's position at the last update
 *   3. up_z = fl(1 - fl(2 fl(fl(qx qx) + fl(qy qy))))  (the z component of the body's z axis);
 *      tilt_count <- up_z < cos_max_tilt ? tilt_count + 1 : 0
 *   4. flag_l = found_l > 0 and fl(fl(fl(Fx Fx) + fl(Fy Fy)) + fl(Fz Fz)) > thr2[l];  airborne_count <- no flag set ? airborne_count + 1 : 0
 *   5. P = sum_a (int32) rint(c_a 2^NMF_TASK_POWER_BITS),  c_a = |fl(f_a qd_a)| clamped: c < 0 ? 0 : (c > power_clip ? power_clip : c)
 *      (an int32 sum: the same whatever the order; a term whose f_a or qd_a is not finite is 0, so nothing that is not finite is
 *      converted);  power = (float) P 2^-NMF_TASK_POWER_BITS  (the conversion rounds to nearest even)
 *   6. n = ep_length + 1;  grace = n <= grace_ticks;  reason = the bits
 *        TILTED when not grace and tilt_count >= tilt_ticks;  AIRBORNE when not grace and airborne_count >= airborne_ticks (the new counts);
 *        HEIGHT when not grace and (z < z_min or z > z_max);  OUT_OF_ARENA when x < arena[0] or x > arena[1] or y < arena[2] or y > arena[3];
 *        GOAL when fl(fl(dx dx) + fl(dy dy)) < goal_radius2,  (dx, dy) = (fl(gx - x), fl(gy - y))  (goal_radius2 = 0: never)
 *      terminated = reason != 0;  truncated = not terminated and n >= max_ticks;  done = terminated or truncated
 *   7. r = alive;  r = fl(r + fl(w_progress progress));  r = fl(r - fl(w_power power));  r = fl(r - fl(w_tilt fl(1 - up_z)));
 *      with GOAL r = fl(r + bonus_goal);  with any other bit r = fl(r - penalty_fail);  reward = r
 *   8. ep_return <- fl(ep_return + reward);  ep_length <- n.  When done: last_return, last_length, last_reason <- ep_return, n, reason
 *      (0: the time limit);  episodes += 1;  successes += 1 with GOAL;  ep_return, ep_length, tilt_count, airborne_count, prev_xy <- 0
 *      and fresh <- 1: the kernel itself starts the next episode.  Otherwise prev_xy <- (x, y), fresh <- 0.
 *   9. obs[w], NMF_TASK_OBS_BODY + 6 + n_q wide.  With the rotation R (body to world) of the unit quaternion, every entry rounded
 *        r00 = fl(1 - fl(2 fl(qy qy + qz qz)))  r01 = fl(2 fl(qx qy - qw qz))          r02 = fl(2 fl(qx qz + qw qy))
 *        r10 = fl(2 fl(qx qy + qw qz))          r11 = fl(1 - fl(2 fl(qx qx + qz qz)))  r12 = fl(2 fl(qy qz - qw qx))
 *        r20 = fl(2 fl(qx qz - qw qy))          r21 = fl(2 fl(qy qz + qw qx))          r22 = up_z
 *      (each product inside rounded first), the row is
 *        [0:3]   -r20, -r21, -r22                                               the direction of gravity in the body frame
 *        [3:6]   fl(fl(fl(r0j vx) + fl(r1j vy)) + fl(r2j vz)),  j = 0, 1, 2     the linear velocity in the body frame
 *        [6:9]   ox, oy, oz                                                     the angular velocity (already in the body frame)
 *        [9:11]  fl(fl(r0j dx) + fl(r1j dy)),  j = 0, 1                         (goal - position, 0) in the body frame, x and y
 *        [11]    z
 *        [12:18] flag_l as 0 / 1
 *        [18:]   fl(fl(ang_k - mean[k]) inv_std[k])                             (the stabilizer's standardisation; inv_std from the host)
 * No square root, no division and no function call: the library's fast-math licences cannot reach the rule (csrc/nmf_exact.h). */
#define NMF_TASK_NONFINITE 1
#define NMF_TASK_TILTED 2
#define NMF_TASK_AIRBORNE 4
#define NMF_TASK_HEIGHT 8
#define NMF_TASK_OUT_OF_ARENA 16
#define NMF_TASK_GOAL 32
#define NMF_TASK_POWER_BITS 10      /* k of step 5: the power sum counts in units of 2^-10                                        */
#define NMF_TASK_MAX_ACT 64
#define NMF_TASK_MAX_Q 256
#define NMF_TASK_OBS_BODY 12        /* the body-level floats at the start of an observation row                                   */
typedef struct nmf_task_params {
  int32_t root_seg;             /* index of the body's root segment in the batch's segment order                                  */
  int32_t n_act, n_q;           /* actuators of the power sum (1..NMF_TASK_MAX_ACT), joint dofs observed (1..NMF_TASK_MAX_Q)       */
  int32_t tilt_ticks, airborne_ticks, max_ticks;   /* each >= 1                                                                    */
  int32_t grace_ticks;          /* >= 0: the first updates of an episode that raise no TILTED, AIRBORNE or HEIGHT                  */
  float cos_max_tilt;           /* in [-1, 1]                                                                                      */
  float z_min, z_max;           /* z_min <= z_max                                                                                  */
  float arena[4];               /* x_min, x_max, y_min, y_max with x_min < x_max and y_min < y_max                                 */
  float goal_radius2;           /* the goal disc's radius squared (>= 0; 0: no goal)                                               */
  float power_clip;             /* >= 0, and n_act rint(power_clip 2^NMF_TASK_POWER_BITS) must fit an int32                        */
  float thr2[6];                /* per leg: the squared force above which a touching leg counts (>= 0)                             */
  float alive, w_progress, w_power, w_tilt, bonus_goal, penalty_fail;
} nmf_task_params;

/* sizeof(nmf_task_params) as this library was compiled (as nmf_eye_params_size). */
size_t nmf_task_params_size(void);

/* An explicit handle for the worlds of `batch`, on its device.  act[n_act] are actuator indices, act_dof[n_act] and obs_dof[n_q]
 * joint dofs (0 = the first after the free joint), mean[n_q] and inv_std[n_q] the standardisation: host arrays, copied.  Owns the
 * per-world arrays and resets every world (nmf_task_reset with a NULL mask); course starts at (1, 0), goal at (0, 0).  NOT
 * stream-ordered (allocations); must not be called inside a stream capture.  NULL on error (nmf_last_error), with nothing left
 * allocated: a null pointer; n_act outside 1..64 or n_q outside 1..256; a parameter, mean or inv_std that is not finite; root_seg,
 * an actuator or a dof outside the model; tilt_ticks, airborne_ticks or max_ticks below 1; grace_ticks below 0; cos_max_tilt outside
 * [-1, 1]; z_min > z_max; an empty arena; goal_radius2 or a thr2 below 0; a power_clip that is negative or lets the power sum
 * overflow; a batch without the six leg sensors; no device memory.  The handle keeps pointers to the batch's arrays: destroy it
 * before the batch. */
nmf_task* nmf_task_create(nmf_batch* batch, const nmf_task_params* params, const int32_t* act, const int32_t* act_dof,
                          const int32_t* obs_dof, const float* mean, const float* inv_std);
void nmf_task_destroy(nmf_task* task);

/* The worlds with mask_dev[w] != 0 (uint8 per world, device memory; NULL: all) get every array below zeroed except course and
 * goal, and fresh = 1: a new episode and empty statistics.  The others are not touched.  Stream-ordered. */
int nmf_task_reset(nmf_task* task, const uint8_t* mask_dev, void* stream);

/* One update of every world: argument checks and ONE kernel launch on `stream`, no allocation, no host synchronisation,
 * hipGraph-capturable (all state lives on the device, so a captured update continues on every replay).  NMF_TASK_DONE is the mask
 * nmf_reset_worlds and every handle's reset take.  Refused: a null handle. */
int nmf_task_update(nmf_task* task, void* stream);

/* Device pointer + row width of an array of the handle (zero-copy views; writable between launches). */
#define NMF_TASK_REWARD 0           /* [1] float32                                                             */
#define NMF_TASK_OBS 1              /* [12 + 6 + n_q] float32                                                  */
#define NMF_TASK_EP_RETURN 2        /* [1] float32                                                             */
#define NMF_TASK_LAST_RETURN 3      /* [1] float32                                                             */
#define NMF_TASK_PREV_XY 4          /* [2] float32                                                             */
#define NMF_TASK_COURSE 5           /* [2] float32: user-written, a unit direction                             */
#define NMF_TASK_GOAL_XY 6          /* [2] float32: user-written                                               */
#define NMF_TASK_TERMINATED 7       /* [1] uint8                                                               */
#define NMF_TASK_TRUNCATED 8        /* [1] uint8                                                               */
#define NMF_TASK_DONE 9             /* [1] uint8                                                               */
#define NMF_TASK_FRESH 10           /* [1] uint8                                                               */
#define NMF_TASK_REASON 11          /* [1] int32: the NMF_TASK_ bits above                                     */
#define NMF_TASK_EP_LENGTH 12       /* [1] int32                                                               */
#define NMF_TASK_LAST_LENGTH 13     /* [1] int32                                                               */
#define NMF_TASK_LAST_REASON 14     /* [1] int32                                                               */
#define NMF_TASK_TILT_COUNT 15      /* [1] int32                                                               */
#define NMF_TASK_AIRBORNE_COUNT 16  /* [1] int32                                                               */
#define NMF_TASK_EPISODES 17        /* [1] int32                                                               */
#define NMF_TASK_SUCCESSES 18       /* [1] int32                                                               */
#define NMF_TASK_FIELD_COUNT 19
void* nmf_task_field_ptr(nmf_task* task, int which, int32_t* width);

/* Odor intensity at n_sensors points rigidly attached to named segments (sensor_seg = index into the
 * batch's segment order, sensor_rel = offset in the segment frame): out[w][d][k] = sum_s peak[s][d] / dist^2.
 * Reads the pose outputs of the last nmf_step / nmf_reset. */
int nmf_odor_intensity(nmf_batch* batch, const int32_t* sensor_seg_dev, const float* sensor_rel_dev, int n_sensors,
                       const float* source_pos_dev, const float* source_peak_dev, int n_sources, int n_dims,
                       float* out_dev, void* stream);

/* Kinematic-replay data path on the device.  Replaces MotionSnippet.get_joint_angles (reference
 * src/flygym_demo/spotlight_data/preprocessing.py:80-142: scipy savgol_filter + interp1d(kind="cubic") on the host):
 * Savitzky-Golay smoothing of the recorded joint angles, the not-a-knot cubic spline through the smoothed frames, its
 * values at t = k * out_dt (k < n_out; the last frame's value beyond the last knot), in float64, stored as float32.
 * clip_dev[n_frames][n_cols] float32; out_dev[n_out][n_cols] float32;
 * sg_taps_dev (float64, device): window interior taps, then window/2 rows of `window` taps for the first window/2 frames
 * (polynomial fit over the first window), then window/2 rows for the last window/2 frames — the constants of
 * savgol_filter(mode="interp"), computed by the caller (flygym_amd.replay.savgol_taps). */
int nmf_replay_resample(const float* clip_dev, int n_frames, int n_cols, double fps, double out_dt,
                        const double* sg_taps_dev, int window, int n_out, float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NMF_H_ */
