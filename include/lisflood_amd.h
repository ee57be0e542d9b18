/*
 * lisflood_amd.h -- C ABI of the MI355X (gfx950) engine for the LISFLOOD per-timestep hot path:
 * kinematic-wave routing, soil-column water balance and LDD-directed reductions.
 *
 * The reference (ec-jrc/lisflood-code v4.3.1) is pure Python and has no FFI of its own; the seams this
 * library sits behind are (paths relative to src/lisflood/hydrological_modules/):
 *   - class kinematicWave                      kinematic_wave_parallel.py:114-184
 *   - numba kernels kinematicRouting/solve1Pixel  kinematic_wave_parallel_tools.py:34-92
 *   - interception_water_balance / soilColumnsWaterBalance   soilloop.py:27-70 / 78-355
 *   - routing.dynamic sub-step arithmetic      routing.py:512-603, 693-703
 *   - np.bincount one-hop upstream sum         routing.py:159-164, lakes.py:215
 * Host code (Python, lisflood-code_amd/lisflood_amd/) binds these entry points with ctypes; the binding
 * a maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: opaque handles, raw pointers and sizes, no exceptions across the boundary;
 *   - every function returns LF_OK (0) or a negative LF_E_* code; lf_last_error() gives the message
 *     (thread-local);
 *   - "pixel order" = the reference's compressed 1-D land-pixel vector, row-major over the land mask
 *     (global_modules/add1.py:268-305); all reals are IEEE fp64;
 *   - pointers named *_host are caller-owned host memory, *_dev are device memory obtained from
 *     lf_device_alloc (or any hipMalloc'ed pointer of the same device);
 *   - there is NO CPU fallback: every compute entry point fails with LF_E_NO_DEVICE when no gfx950
 *     device is usable;
 *   - execution model: one HIP stream per device, every entry point enqueues on it and returns (only the *_host
 *     forms, lf_memcpy_* and lf_device_synchronize wait); per-device scratch (soil work lists, router buffers) is
 *     not locked, so drive a device from ONE host thread -- use one process per GPU for multi-GPU work, as
 *     bench.py does.
 */
#ifndef LISFLOOD_AMD_H
#define LISFLOOD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LF_OK 0
#define LF_E_INVALID (-1)   /* bad argument */
#define LF_E_CYCLE (-2)     /* LDD has a cycle (the reference loops forever: kinematic_wave_parallel.py:99) */
#define LF_E_NO_DEVICE (-3) /* no usable HIP device */
#define LF_E_HIP (-4)       /* HIP runtime error, see lf_last_error() */
#define LF_E_SECTION (-5)   /* section not in {main_channel, floodplains} / floodplains not configured
                               (kinematic_wave_parallel.py:172) */
#define LF_E_COMM (-6)      /* RCCL error */

#define LF_SECTION_MAIN 0        /* "main_channel" */
#define LF_SECTION_FLOODPLAINS 1 /* "floodplains"  */

typedef struct lf_graph lf_graph;   /* host: LDD -> adjacency -> routing orders            */
typedef struct lf_router lf_router; /* device: one kinematicWave instance                   */
typedef struct lf_dist_graph lf_dist_graph;   /* host: one rank's row block of the raster, with halos */
typedef struct lf_dist_router lf_dist_router; /* device: one rank's share of a partitioned kinematicWave */
typedef struct lf_comm lf_comm;               /* RCCL communicator (one rank per GPU)            */

const char *lf_last_error(void);
int lf_version(void);
/* sizeof(lf_substep_args), sizeof(lf_interception_args), sizeof(lf_soil_args), sizeof(lf_canopy_args),
 * sizeof(lf_surface_args), sizeof(lf_inloop_args), sizeof(lf_pixel_args): lets a binding verify its struct mirrors. */
int lf_struct_sizes(int64_t out[7]);

/* ---------------------------------------------------------------------------------------------
 * device plumbing
 * ------------------------------------------------------------------------------------------- */
int lf_device_count(int *count);
int lf_device_name(int device, char *buf, size_t buflen); /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
int lf_device_alloc(int device, size_t bytes, void **ptr_dev);
int lf_device_free(int device, void *ptr_dev);
int lf_memcpy_h2d(int device, void *dst_dev, const void *src_host, size_t bytes);
/* the same without waiting: the bytes are copied to a page-locked staging slot owned by the library (the source is free
 * again on return) and go up by DMA on the stream the library calls currently go to, in order with the kernels around it.
 * For small per-step vectors (inflow hydrographs, LAI): lf_memcpy_h2d's wait for the stream would stall the host. */
int lf_memcpy_h2d_staged(int device, void *dst_dev, const void *src_host, size_t bytes);
/* Page-locked host memory for the vectors that cross PCIe every model step (the meteorological forcing, which the
 * reference reads from netCDF into fresh arrays each step, Lisflood_dynamic.py:84-112): a copy from such a buffer is a
 * true asynchronous DMA at the link's rate; from pageable memory the runtime stages it and blocks the caller (measured
 * at 5000^2: 1 GB of forcing per step, 29 GB/s pageable -- longer than the step's kernels).  lf_host_alloc fails
 * without a HIP device like every other entry point. */
int lf_host_alloc(int device, size_t bytes, void **ptr_host);
int lf_host_free(int device, void *ptr_host);
/* Double-buffered uploads on a second HIP stream, so that the copies of the NEXT step's inputs overlap the kernels of
 * the current step.  For buffer set b in {0, 1}:
 *     lf_upload_begin(b); lf_upload_copy(...) ...; lf_upload_end(b)            -- at any time, e.g. right after a step
 *     lf_compute_acquire(b); <entry points whose kernels read set b>; lf_compute_release(b)
 * The copies wait for the kernels that last read set b, those kernels wait for the copies; the other set is free. */
int lf_upload_begin(int device, int set);
int lf_upload_copy(int device, void *dst_dev, const void *src_host, size_t bytes);
/* the same for a vector the caller holds as float32 (the reference's meteo files are float32; readnetcdf widens them on the
 * host): half the bytes over PCIe, widened to fp64 on the device behind the copy -- the same exact conversion */
int lf_upload_copy_f32(int device, double *dst_dev, const float *src_host, size_t count);
/* the same for the member rows of an ensemble's forcing vector, which the caller holds in PIXEL order: for r < rows, i < n
 *     dst[r * dst_stride + i] = (double)src[(src_rows == 1 ? 0 : r) * n + (index_dev ? index_dev[i] : i)]
 * src_host: src_rows x n dense values, float32 if src_f32 = 1, float64 if 0; src_rows is 1 (one row for every member) or
 * rows.  The raw image goes up by ONE asynchronous copy into a staging buffer kept per destination (grow-only, freed with
 * the destination and by lf_device_trim; shared with lf_upload_copy_f32); a kernel on the copy stream behind it gathers
 * through the index table (position -> pixel, on the device; NULL: identity), widens and writes the rows -- no host
 * permutation, no host widening, no padded host image.  Elements n .. dst_stride - 1 of a row are never written.
 * LF_E_INVALID, with the argument named, before a device is touched: rows < 1, src_rows not 1 or rows, src_f32 not 0 / 1,
 * n < 0 or beyond the 32-bit range of a launch, dst_stride < n, dst_dev or src_host NULL with n > 0. */
int lf_upload_rows(int device, double *dst_dev, int64_t dst_stride, int rows, const void *src_host, int src_rows, int src_f32,
                   int64_t n, const int32_t *index_dev);
int lf_upload_end(int device, int set);
/* host side of the protocol: blocks until the copies of the last lf_upload_begin(set) .. lf_upload_end(set) have finished.
 * Call it before refilling, in place, a page-locked source buffer that was handed to lf_upload_copy for `set` (the copy is
 * a true asynchronous DMA out of that buffer); returns at once if the set was never uploaded. */
int lf_upload_wait(int device, int set);
int lf_compute_acquire(int device, int set);
int lf_compute_release(int device, int set);
/* The mirror image for results: double-buffered downloads on a stream of their own (not the upload stream: both DMA
 * directions run at once), so that a report map leaves the device beside the kernels of the NEXT step.  For set b in {0, 1}:
 *     lf_report_acquire(b)   -- the stream the library calls currently go to waits until the last download out of set b's
 *                               device staging has finished: a kernel enqueued next may overwrite that staging
 *     <lf_pack_rasters_device into set b's staging>
 *     lf_download_begin(b)   -- the download stream waits for everything issued so far on the main and on the side stream
 *     lf_download_copy(dst_host, src_dev, bytes) ...   -- asynchronous device-to-host copies; dst_host from lf_host_alloc
 *     lf_download_end(b)     -- records the set's event
 *     lf_download_wait(b)    -- the host blocks until that event; returns at once if the set was never downloaded
 * Only lf_download_wait blocks the host.  lf_device_synchronize waits for the download stream too; lf_device_trim releases
 * the stream and its events (made again on next use).  LF_E_INVALID with a message: a set other than 0 or 1, _begin while a
 * set is open or between lf_lane_fork and lf_lane_join, _copy or _end outside a _begin / _end pair, _end of another set than
 * the open one, _copy with a NULL pointer and bytes > 0. */
int lf_report_acquire(int device, int set);
int lf_download_begin(int device, int set);
int lf_download_copy(int device, void *dst_host, const void *src_dev, size_t bytes);
int lf_download_end(int device, int set);
int lf_download_wait(int device, int set);
/* A second compute stream for a part of a step that the first kernels of the NEXT step do not depend on (the channel
 * wavefront of a model step beside the canopy / soil / overland kernels of the step after it): between _begin and _end every
 * library call of this device goes to the side stream, behind what the main stream holds so far; after _end the side work
 * stays in flight beside the main stream.  _join: the main stream waits for the side work issued so far; the copy entry
 * points (lf_memcpy_*) join by themselves, lf_device_synchronize waits for both streams. */
int lf_side_stream_begin(int device);
int lf_side_stream_end(int device);
int lf_side_stream_join(int device);
/* Lanes: several streams of one device for work items that do not depend on one another -- the blocks of a row-block
 * partition that live on ONE GPU are independent inside a phase (on real hardware each has its own GPU):
 *     lf_lane_fork(); for k: { lf_lane_select(k + 1); <block k's calls> }  lf_lane_select(0); lf_lane_join();
 * a lane first waits for what the main stream held at the fork; the join makes the main stream wait for every lane used. */
int lf_lane_fork(int device);
int lf_lane_select(int device, int lane);
int lf_lane_join(int device);
/* releases what the context keeps for reuse (lane streams, fp32 staging buffers, the staging arena of the *_host forms, the
 * download stream and its events);
 * waits for the device first, refuses between lf_lane_fork and lf_lane_join or inside a side section */
int lf_device_trim(int device);
int lf_memcpy_d2h(int device, void *dst_host, const void *src_dev, size_t bytes);
int lf_memcpy_d2d(int device, void *dst_dev, const void *src_dev, size_t bytes);
int lf_memset(int device, void *dst_dev, int value, size_t bytes);
int lf_device_synchronize(int device);
/* hipEvent stopwatch on the library's compute stream of `device` (the stream every kernel of this
 * library is launched on): start records an event, stop records another, synchronises and returns the
 * elapsed milliseconds. */
int lf_timer_start(int device);
int lf_timer_stop(int device, double *elapsed_ms);

/* profiling aid: stream copy of n doubles with bytes_per_lane in {8, 16}; its HBM traffic is exactly
 * n*8 B read + n*8 B written, which calibrates rocprofv3's FETCH_SIZE / WRITE_SIZE on gfx950. */
int lf_calibration_copy(int device, const double *src_dev, double *dst_dev, int64_t n, int bytes_per_lane);
/* nread (1..8) read streams + one write stream of n doubles each (dst[i] = src_0[i] + ... ), 8 bytes per lane: the byte
 * mix of the level sweep without its arithmetic -- the bandwidth ceiling of a kernel with that many streams. */
int lf_calibration_streams(int device, int nread, const double *const *src_dev, double *dst_dev, int64_t n);

/* ---------------------------------------------------------------------------------------------
 * graph: replaces rebuildFlowMatrix/decodeFlowMatrix/streamLookups/topoDistFromSea/_setRoutingOrders
 * (kinematic_wave_parallel.py:59-106, 140-158; kinematic_wave_parallel_tools.py:111-130)
 * ------------------------------------------------------------------------------------------- */
/* ldd_codes: N compressed LISFLOOD keypad codes (doubles, as the reference passes them; 0 = sea,
 * 5 = pit; any value outside {1,2,3,4,6,7,8,9} is "no flow").  land_mask: H*W bytes, non-zero = land. */
int lf_graph_create(const double *ldd_codes, const uint8_t *land_mask, int H, int W, lf_graph **out);
/* same, with zero-length links for the structures of the routing loop: virtual_down[N] (may be NULL; -1 = none)
 * names, for a pit u of THIS (cut) LDD, the pixel v it drains into in the uncut LDD (structures.py:44-61 cuts the
 * LDD just upstream of lakes and reservoirs; routing.py:159-164 keeps the uncut link in `downstruct`).  u gets the
 * same level as v, which is what lets lf_routing_substeps_fused_structures run lakes.py / reservoir.py between two
 * launches of the wavefront.  Levels then differ from the reference's routing orders; router results do not. */
int lf_graph_create_ex(const double *ldd_codes, const uint8_t *land_mask, int H, int W, const int64_t *virtual_down,
                       lf_graph **out);
/* linked[N], by engine position: 1 = the cell is such a zero-length link (it sits at the end of its level, outside
 * every upstream range) */
int lf_graph_get_links(const lf_graph *g, uint8_t *linked);
/* The site plan of the time-major form of lf_routing_substeps_fused_structures, host arrays only (no device): n cells
 * in nlevels levels (level_start[nlevels + 1], as lf_graph_get_layout gives it) and the six site lists of lf_inloop_args
 * in engine positions.  Out: feed_slot[n] -- entry e of lake_ups_idx has slot e, entry e of res_ups_idx slot
 * lake_ups_ptr[n_lakes] + e, feed_slot is the inverse map (-1: the cell feeds no site); level_site[level_site_ptr[k] ..
 * level_site_ptr[k + 1]) -- the sites (lakes 0 .. n_lakes - 1, then the reservoirs) whose cell is on level k, ascending
 * (level_site_ptr[nlevels + 1], level_site[n_lakes + n_res]); *applies = 0 when a site cell feeds another site, two sites
 * share a cell, a cell feeds two sites or a feeder is not on its site's level: the call then runs the skewed wavefront,
 * and the arrays are not complete.  A cell or a pointer out of range is LF_E_INVALID. */
int lf_site_plan(int64_t n, int nlevels, const int64_t *level_start, int64_t n_lakes, const int32_t *lake_cell,
                 const int32_t *lake_ups_ptr, const int32_t *lake_ups_idx, int64_t n_res, const int32_t *res_cell,
                 const int32_t *res_ups_ptr, const int32_t *res_ups_idx, int32_t *applies, int32_t *feed_slot,
                 int32_t *level_site_ptr, int32_t *level_site);
/* raster form for large domains: H*W uint8 codes; land_mask may be NULL (= all land). */
int lf_graph_create_raster(const uint8_t *ldd_raster, const uint8_t *land_mask, int H, int W, lf_graph **out);
void lf_graph_destroy(lf_graph *g);
int64_t lf_graph_num_pixels(const lf_graph *g);   /* N  */
int64_t lf_graph_num_levels(const lf_graph *g);   /* NL = order_start_stop.shape[0] */
int lf_graph_max_upstream(const lf_graph *g);     /* K  = upstream_lookup.shape[1]  */
/* the reference's attributes, for parity tests: downstream_lookup[N] (float64, -1 = none),
 * upstream_lookup[N*K] (int64, -1 filled, ascending source id), num_upstream_pixels[N] */
int lf_graph_get_lookups(const lf_graph *g, double *downstream, int64_t *upstream, int64_t *num_upstream);
/* pixels_ordered[N], order_start_stop[NL*2] (kinematic_wave_parallel.py:150-158) */
int lf_graph_get_orders(const lf_graph *g, int64_t *pixels_ordered, int64_t *order_start_stop);
/* engine layout: perm[N] = pixel at sweep position p (levels ascending; inside a level, breadth-first
 * from the outlets so that the upstream cells of position p are the contiguous positions
 * [ups_ptr[p], ups_ptr[p+1])); level_start[NL+1]. */
int lf_graph_get_layout(const lf_graph *g, int32_t *perm, int32_t *ups_ptr, int64_t *level_start);

/* ---------------------------------------------------------------------------------------------
 * router: replaces class kinematicWave (kinematic_wave_parallel.py:114-184)
 * ------------------------------------------------------------------------------------------- */
/* alpha[N]; dx[N] or NULL + dx_scalar; alpha_floodplains[N] or NULL (no split routing). */
int lf_router_create(const lf_graph *g, const double *alpha, double beta, const double *dx, double dx_scalar,
                     double dt, const double *alpha_floodplains, int device, lf_router **out);
void lf_router_destroy(lf_router *r);
int lf_router_device(const lf_router *r);
int64_t lf_router_num_pixels(const lf_router *r);
/* kinematicWaveRouting(discharge, specific_lateral_inflow, section): discharge[N] is updated in place.
 * Host-buffer form (PCIe-inclusive): H2D, route, D2H. */
int lf_router_route_host(lf_router *r, double *discharge_host, const double *lateral_host, int section);
/* Device-resident form: discharge_dev[N] (in/out) and lateral_dev[N] in pixel order, asynchronous on the
 * library stream. */
int lf_router_route_device(lf_router *r, double *discharge_dev, const double *lateral_dev, int section);
/* `count` (<= 4) routers built on ONE graph -- surface_routing.py:108-113 builds the direct / other / forest overland
 * routers on the same LDD, and calls them one after the other (:151-153) -- swept together: one launch per level for
 * all of them instead of one per router.  engine_order != 0: vectors in sweep order (lf_router_route_ordered).  Routers
 * with different level schedules are simply swept one after the other. */
int lf_router_route_device_multi(int count, lf_router **routers, double **discharge_dev, const double **lateral_dev,
                                 int section, int engine_order);
/* Engine-order form.  The engine's HBM layout of a per-pixel vector is "sweep order" (levels ascending,
 * breadth-first inside a level; lf_graph_get_layout's perm): in that layout every access of the sweep is
 * a coalesced stream and discharge is updated in place.  Element-wise work (routing.dynamic's fix-ups,
 * sideflow assembly) is order-agnostic, so a model step can keep all its vectors in engine order and
 * convert only at its boundary with these two permutations (dst[p] = src[perm[p]] and its inverse). */
/* dst[i] = src[index[i]], i < n: permutation between two domains (e.g. full-raster pixel order -> engine order of a
 * router that covers a subset of the pixels) */
int lf_gather_device(int device, int64_t n, const int32_t *index_dev, const double *src_dev, double *dst_dev);
int lf_router_to_engine_order(lf_router *r, const double *src_pix_dev, double *dst_ord_dev);
int lf_router_from_engine_order(lf_router *r, const double *src_ord_dev, double *dst_pix_dev);
/* (The first such call of a router with per-pixel channel lengths builds, per section, a 16-byte (alpha*dx/dt, dx) record per
 * cell on the device for its wide levels -- 16 N bytes that stay with the router; LF_LEVEL_STATICS=0 keeps the two vectors.) */
int lf_router_route_ordered(lf_router *r, double *discharge_ord_dev, const double *lateral_ord_dev, int section);
/* `members` (>= 1) state vectors of ONE router swept together: member m's discharge (in/out) is
 * discharge_ord_dev + m * stride, its lateral inflow lateral_ord_dev + m * stride, both in sweep order,
 * stride >= N in elements.  One launch per wide level / narrow run / level block for all members; each
 * member's result is bit-identical to lf_router_route_ordered on that member alone.  Elements between N
 * and stride are neither read nor written.  (General exponent: the router's `constant` grows to members * N.) */
int lf_router_route_ordered_members(lf_router *r, double *discharge_ord_dev, const double *lateral_ord_dev,
                                    int members, int64_t stride, int section);
/* The same for `count` (1 to 4) routers at once -- the three overland routers of an ensemble: router i sweeps its own
 * [members][stride] rows discharge_ord_dev[i] / lateral_ord_dev[i].  Routers that lf_router_route_device_multi would sweep
 * together (same graph and schedule, same device, no links, not profiling) share every launch: one per wide level / narrow
 * run / level block for all count * members (router, member) units (general exponent: one preparing launch for all units,
 * each router's `constant` grows to members * N; more units than a grid's second dimension holds: in slices of members).
 * Other routers get one lf_router_route_ordered_members call each.  Every (router, member) row is bit-identical to
 * lf_router_route_ordered on that router with that row alone.  count, members and stride are checked before a router or a
 * device is touched. */
int lf_router_route_ordered_members_multi(int count, lf_router **routers, double **discharge_ord_dev,
                                          const double **lateral_ord_dev, int members, int64_t stride, int section);
/* dst[r * dst_stride + i] = src[r * src_stride + index[i]], i < n, r < rows: lf_gather_device for `rows` rows with one index
 * table in one launch (each member's ToChanM3RunoffDt from the overland order into the channel router's engine order).
 * dst_stride >= n; the elements between the rows of dst are not written. */
int lf_gather_rows_device(int device, int64_t n, const int32_t *index_dev, const double *src_dev, int64_t src_stride,
                          double *dst_dev, int64_t dst_stride, int rows);
/* Products over the members of an ensemble, element by element (lf_members.hip).  Both calls read `members` rows of n
 * doubles, `stride` elements apart (elements between n and stride are never read); the value of (m, i) is
 * rows_dev[m * stride + i] / divisor, an IEEE division (divisor = NoRoutSteps on sumDisDay: the bits of ChanQAvg; 1.0: the
 * element itself).  The results of element i go to index dst_index_dev ? dst_index_dev[i] : i of outputs dst_n long
 * (dst_index_dev: int32 in device memory, injective -- the caller's word); what no i maps to is not written.  Asynchronous
 * on the device's library stream, like lf_gather_rows_device.
 * lf_members_summary_device, in ONE pass over the members in ascending order, every output that is not NULL:
 *   mean   ((x0 + x1) + x2) + ... in that order, divided by (double)members;
 *   min / max  folds with the accumulator first (np.minimum / np.maximum): a NaN sticks, on a tie (-0.0 against +0.0 too)
 *          the earlier member stays;
 *   exceed [n_thresholds][dst_n] int32: the members with x > thresholds_dev[t * threshold_stride + i] (a NaN on either side
 *          does not count), for up to 4 threshold rows in the order of the source rows.
 * lf_members_order_statistics_device: out_dev[r * dst_n + .] is the value with exactly ranks_host[r] values before it when
 * a goes before b if a < b or b is a NaN and a is none, and otherwise the lower member goes first -- np.sort(x, axis=0,
 * kind="stable")[rank]; the value itself, so the sign of a zero survives.  Up to 8 ranks (a host array), up to 128 members:
 * an element's column sits in LDS, 256 lanes per workgroup up to 32 members, 128 up to 64, 64 up to 128.
 * LF_E_INVALID, with the argument named, before a device is touched: members < 1, n < 0 or beyond the 32-bit range of a
 * launch, stride < n, dst_n != n without a dst_index_dev, dst_n < n, n_thresholds outside 0..4, thresholds without
 * thresholds_dev and exceed_dev or with threshold_stride < n, no output at all, n_ranks outside 1..8, a rank outside
 * [0, members), members > 128 (order statistics), rows_dev or out_dev NULL with n > 0.  n == 0: LF_OK, nothing is launched. */
int lf_members_summary_device(int device, const double *rows_dev, int members, int64_t stride, int64_t n, double divisor,
                              const int32_t *dst_index_dev, int64_t dst_n, double *mean_dev, double *min_dev, double *max_dev,
                              int n_thresholds, const double *thresholds_dev, int64_t threshold_stride, int32_t *exceed_dev);
int lf_members_order_statistics_device(int device, const double *rows_dev, int members, int64_t stride, int64_t n,
                                       double divisor, const int32_t *dst_index_dev, int64_t dst_n, int n_ranks,
                                       const int32_t *ranks_host, double *out_dev);
/* Products over the steps of a run, per member and element: one call folds the step's member rows (the same rows, stride,
 * divisor and value v = rows_dev[m * stride + i] / divisor as above) into accumulators that stay on the device.  Accumulator
 * rows are track_stride elements apart, in the order of the source rows: peak_dev[m * track_stride + i], and the thresholded
 * ones [n_thresholds][members] rows, first_above_dev[(t * members + m) * track_stride + i]; the thresholds are shared by the
 * members, thresholds_dev[t * threshold_stride + i].  Elements between n and a stride are neither read nor written, in the
 * sources and the accumulators alike.  Every output pointer may be NULL and is then skipped (peak_step_dev needs peak_dev).
 * first != 0 reads no accumulator:
 *   peak = v, peak_step = step, sum = v, first_above[t] = v > thr[t] ? step : -1, steps_above[t] = v > thr[t] ? 1 : 0.
 * first == 0:
 *   take = v > peak || (v != v && peak == peak);  peak = take ? v : peak;  peak_step = take ? step : peak_step
 *          (np.maximum with the accumulator first: a NaN sticks from the step it arrives, on a tie -- -0.0 against +0.0
 *          too -- the earlier step stays);
 *   sum = sum + v: one addition per call, the sum is in call order;
 *   with a = v > thr[t] (false with a NaN on either side):
 *          first_above[t] = (a && steps_above[t] == 0) ? step : first_above[t];  steps_above[t] += a
 *          (without steps_above_dev the test is first_above[t] < 0).
 * step is the caller's number of this update, >= 0 (-1 marks "never"); the library keeps no counter.  Asynchronous on the
 * stream the library calls currently go to.  One lane per element, every (member, element) has one owner; a value that does
 * not change is not stored, peak_step and (with steps_above_dev) first_above are never loaded: 32 + 8 n_thresholds bytes per
 * (member, element) at most with every output.
 * LF_E_INVALID, with the argument named, before a device is touched: members < 1, n < 0 or beyond the 32-bit range of a
 * launch, stride < n, rows_dev NULL with n > 0, track_stride < n, step < 0, n_thresholds outside 0..4, thresholds without
 * thresholds_dev, with threshold_stride < n or with both first_above_dev and steps_above_dev NULL, peak_step_dev without
 * peak_dev, no output at all.  n == 0: LF_OK, nothing is launched. */
int lf_members_track_device(int device, const double *rows_dev, int members, int64_t stride, int64_t n, double divisor,
                            int step, int first, int64_t track_stride,
                            double *peak_dev, int32_t *peak_step_dev, double *sum_dev,
                            int n_thresholds, const double *thresholds_dev, int64_t threshold_stride,
                            int32_t *first_above_dev, int32_t *steps_above_dev);
/* The analysis step of an ensemble (EnKF / ETKF / smoother update, particle resampling), element by element and IN PLACE on
 * `members` rows of n doubles, `stride` elements apart; elements between n and stride are neither read nor written.
 * Asynchronous on the stream the library calls currently go to; no allocation, no synchronisation, no atomics, no scratch.
 * lf_members_transform_device: with x[k] = rows_dev[k * stride + i] as it was BEFORE the call, for every output member m
 *   t = x[0] * W[0][m];  for k = 1 .. members - 1:  t = t + x[k] * W[k][m]     (one multiply, one add, ascending k; never fused)
 *   v = taper_dev ? x[m] + taper_dev[i] * (t - x[m]) : t
 *   lo = lower_dev ? lower_dev[i] : lower;   v = (lo > v || (lo != lo && v == v)) ? lo : v
 *   hi = upper_dev ? upper_dev[i] : upper;   v = (hi < v || (hi != hi && v == v)) ? hi : v
 *   rows_dev[m * stride + i] = v
 * W[k][m] = weights_dev[k * members + m], one [members][members] table in device memory for the whole domain; taper_dev,
 * lower_dev and upper_dev are [n] rows shared by the members, or NULL (no taper; the scalar bound).  A scalar bound of
 * -inf / +inf leaves every bit of v (-0.0 and NaN included); a NaN bound makes every non-NaN v a NaN.  The identity matrix
 * is NOT a bit-exact no-op: a -0.0 comes back as +0.0 unless every other member of its column has its sign bit set (the
 * other members' products are zeros of their own sign), and a column with an inf or a NaN becomes NaN in every other member
 * (0 * inf) -- with one member nothing is added and every bit stays.  A selection matrix is therefore no substitute for
 * lf_members_resample_device.  Up to 64 members (the table is 32 KiB, read through the scalar cache).  A lane owns its
 * element's whole column, which sits in LDS before the first store; 256 lanes per workgroup up to 32 members, 128 up to 64.
 * lf_members_resample_device: rows_dev[m * stride + i] = x[parents_host[m]], a copy of the bits.  parents_host: int32
 * [members] on the host, read before the call returns.  A row with parents_host[m] == m is not written, and read only where
 * another row draws from it; with the identity nothing is launched.  Up to 128 members.
 * LF_E_INVALID, with the argument named, before a device is touched: rows_dev, weights_dev or parents_host NULL,
 * members < 1 or above the call's limit, n < 0 or beyond the 32-bit range of a launch, stride < n with members > 1, a parent
 * outside 0 .. members - 1, lower > upper where both are scalars.  n == 0: LF_OK, nothing is launched. */
int lf_members_transform_device(int device, double *rows_dev, int members, int64_t stride, int64_t n,
                                const double *weights_dev, const double *taper_dev,
                                const double *lower_dev, double lower, const double *upper_dev, double upper);
int lf_members_resample_device(int device, double *rows_dev, int members, int64_t stride, int64_t n,
                               const int32_t *parents_host);
/* The localised serial analysis (the two-step ensemble filter of Anderson 2003 / Whitaker & Hamill 2002 with Gaspari-Cohn
 * localisation): the observation-space increments of ALL gauges regressed onto every element in ONE pass, IN PLACE on
 * `members` (2 .. 64) rows of n doubles, `stride` elements apart, as lf_members_transform_device takes them.  cx_dev, cy_dev:
 * [n] doubles, the coordinates of the elements.  table_dev: gauges * (2 * members + 5) doubles in device memory, G = gauges
 * (1 .. 256), M = members, in sections
 *   A[G][M] anomalies | D[G][M] increments | s[G] = 1 / sum_k A[j][k]^2 | gx[G] | gy[G] gauge coordinates |
 *   c[G] half-width, > 0 | cut2[G] = (2.0 * c) * (2.0 * c)
 * which the host makes in observation space (lisflood_amd.assimilation.serial_increments).  With x[k] = rows_dev[k * stride + i],
 * for every element i the gauges are taken in ascending j, each on the column as the gauges before it left it:
 *   dx = cx[i] - gx[j];  dy = cy[i] - gy[j];  d2 = dx * dx + dy * dy
 *   if !(d2 < cut2[j]): the gauge leaves the element alone (every member keeps its bits)
 *   z = sqrt(d2) / c[j]                                                        (IEEE square root and division)
 *   z <= 1:  p = -0.25 * z + 0.5;  p = p * z + 0.625;  p = p * z - C53;  p = p * z;  rho = p * z + 1.0
 *   else:    q = C112 * z - 0.5;  q = q * z + 0.625;  q = q * z + C53;  q = q * z - 5.0;  q = q * z + 4.0;  rho = q - C23 / z
 *            with the double constants C53 = 5.0 / 3.0, C112 = 1.0 / 12.0, C23 = 2.0 / 3.0
 *   if !(rho > 0): the gauge leaves the element alone (rho reaches about -3e-16 just below z = 2; a NaN coordinate, whose
 *            d2 is no less than anything, has left at the first test)
 *   cov = x[0] * A[j][0];  for k = 1 .. M - 1:  cov = cov + x[k] * A[j][k]     (one multiply, one add, ascending k; never fused)
 *   g = rho * (cov * s[j])
 *   for k = 0 .. M - 1:  x[k] = x[k] + g * D[j][k]
 * and after the last gauge the bound lines of lf_members_transform_device (lower, then upper) and the store.  The covariance
 * is taken WITHOUT centring x: sum_k x[k] A[j][k] equals sum_k (x[k] - mean) A[j][k] only because the host's anomalies sum
 * to zero to rounding, which is the caller's to keep.  Bounds apply to every element, touched by a gauge or not; a call
 * without bounds (both rows NULL, lower = -inf, upper = +inf) stores nothing to an element that no gauge touched, so -0.0
 * and every NaN payload stay there.  Elements n .. stride - 1 are neither read nor written; the table is only read.  A lane
 * owns its element's whole column, which stays on chip from the load to the store (in registers up to 16 members; beyond
 * that in LDS, 256 lanes per workgroup up to 32 members, 128 up to 64); the table is read through the scalar cache, and a gauge with no lane of a wavefront in range costs that
 * wavefront one distance and one vote.  Asynchronous on the stream the library calls currently go to; no allocation, no
 * synchronisation, no atomics, no scratch.  16 members + 16 bytes per element at most, about 4 members + 40 fp64 operations
 * per element and gauge in range (measured: profiles/members_regress.json).
 * LF_E_INVALID, with the argument named, before a device is touched: members outside 2 .. 64, gauges outside 1 .. 256, n < 0
 * or beyond the 32-bit range of a launch, stride < n, rows_dev, cx_dev, cy_dev or table_dev NULL with n > 0, lower > upper
 * where both are scalars.  n == 0: LF_OK, nothing is launched. */
int lf_members_regress_device(int device, double *rows_dev, int members, int64_t stride, int64_t n, int gauges,
                              const double *cx_dev, const double *cy_dev, const double *table_dev,
                              const double *lower_dev, double lower, const double *upper_dev, double upper);
/* The forecast half of the cycle: what makes the members differ.  Member rows (forcing, or state as model error / jitter)
 * perturbed from `rank` static spatial patterns on the device and a [members][rank] table of coefficients from the host --
 * only the table crosses PCIe.  For every element i < n and member m < members
 *   s = c[m][0] * P[0][i];   for r = 1 .. rank-1:  s = s + c[m][r] * P[r][i]      (one multiply, one add, ascending r; never fused)
 *   b = base_dev ? base_dev[i] : rows_dev[m*stride + i]                          (as it was BEFORE the call)
 *   v = multiplicative ? b * (1.0 + s) : b + s
 *   lo = lower_dev ? lower_dev[i] : lower;   v = (lo > v || (lo != lo && v == v)) ? lo : v
 *   hi = upper_dev ? upper_dev[i] : upper;   v = (hi < v || (hi != hi && v == v)) ? hi : v
 *   rows_dev[m*stride + i] = v
 * P[r][i] = patterns_dev[r*pattern_stride + i] (device); c[m][r] = coeff_host[m*rank + r], HOST memory, read before the call
 * returns (the source is free again on return, like parents_host): the table goes up through a page-locked slot of the
 * library (as lf_memcpy_h2d_staged does) into one of four tables kept on the device, on the call's own stream.  lower_dev /
 * upper_dev: [n] rows shared by the members, or NULL (the scalar bound); the bound lines are lf_members_transform_device's.
 * Elements n .. stride-1 of a row are neither read nor written.  base_dev: one [n] row for every member, or NULL (every
 * member's own row, in place).  base_dev may be rows_dev itself -- member 0's row, which is how a forcing vector that went up
 * as one row is spread over the members: a lane owns element i of every member and has read b before its first store, so
 * the in-place form is safe.  Consequences: all-zero coefficients under `multiplicative` leave every non-NaN bit of b, -0.0
 * included (s = +0.0, 1.0 + s = 1.0, b * 1.0 = b), before the bounds; in additive mode -0.0 + (+0.0) is +0.0, so zero
 * coefficients are no bit-exact no-op there; 0 * inf in a pattern gives NaN (a zero coefficient does not switch an infinite
 * pattern value off).  Up to 128 members, rank up to 16 (the table: 16 KiB, read through the scalar cache).
 * lf_members_perturb_device is asynchronous on the stream the library calls currently go to (main, side or lane).
 * lf_upload_perturb_rows runs on the copy stream and is legal only between lf_upload_begin(set) and lf_upload_end(set), where
 * it runs behind the lf_upload_rows of the same destination.  Neither allocates per call (the four tables are made on first
 * use), neither synchronises the host; no atomics, no LDS, no scratch.  Traffic per element: 8 (rank + 1 + members) bytes with
 * a base row, 8 (rank + 2 members) in place, plus 8 per bound row; 2 rank + 2 unfused fp64 operations per store.  Measured
 * (MI355X, 4e6 elements, rank 8, 4 / 16 / 51 members; profiles/members_perturb.json): 0.077 / 0.159 /
 * 0.323 ms from one base row and 0.097 / 0.249 / 0.600 ms in place, 0.80 - 0.94 of the 6.29 TB/s copy ceiling; a prefetched
 * ensemble step with two forcing vectors spread this way takes what it takes on [n] forcing alone, within its spread.
 * LF_E_INVALID, with the argument named, before a device is touched: rows_dev, patterns_dev or coeff_host NULL, members < 1
 * or > 128, rank < 1 or > 16, n < 0 or beyond the 32-bit range of a launch, stride < n with members > 1, pattern_stride < n with
 * rank > 1, multiplicative not 0 or 1, lower > upper where both are scalars.  lf_upload_perturb_rows outside an open upload
 * section: LF_E_INVALID.  n == 0: LF_OK, nothing is launched. */
int lf_members_perturb_device(int device, double *rows_dev, int members, int64_t stride, int64_t n,
                              const double *base_dev,
                              int rank, const double *patterns_dev, int64_t pattern_stride,
                              const double *coeff_host, int multiplicative,
                              const double *lower_dev, double lower, const double *upper_dev, double upper);
int lf_upload_perturb_rows(int device, double *rows_dev, int members, int64_t stride, int64_t n,
                           const double *base_dev,
                           int rank, const double *patterns_dev, int64_t pattern_stride,
                           const double *coeff_host, int multiplicative,
                           const double *lower_dev, double lower, const double *upper_dev, double upper);
/* Sums ACROSS the elements of member rows -- zonal sums: a footprint, a basin, a member's total storage -- in a fixed order,
 * so that the fp64 result is reproducible bit for bit (lisflood_amd.zonal.ZonePlan fixes the order on the host; no atomics
 * anywhere).  ONE call is ONE pass: it sums `runs` runs of consecutive entries, run r = entries run_start_dev[r] ..
 * run_start_dev[r + 1] - 1 (int32 [runs + 1] in device memory, ascending, at most 256 entries per run, run_start_dev[runs] <=
 * entries -- the caller's word), for every member m < members:
 *   entry e reads   x = rows_dev[m * stride + (index_dev ? index_dev[e] : e)]     (index_dev: int32 [entries] on the device)
 *   its value is    t = divisor == 1.0 ? x : x / divisor                           (an IEEE division)
 *                   t = weights_dev ? t * weights_dev[e] : t                       (one multiply, rounded on its own)
 *   the run's values v[0 .. len) are padded to 256 with +0.0 -- a selected +0.0, never a product, and nothing is loaded for it;
 *   lane l of 64:   s = 0.0;  s = s + v[l];  s = s + v[l + 64];  s = s + v[l + 128];  s = s + v[l + 192]
 *   for d = 32, 16, 8, 4, 2, 1:   s[l] = s[l] + s[l + d]  for l < d
 *   out_dev[m * out_stride + r] = s[0]
 * so a run of length 0 gives +0.0, a -0.0 alone in a run gives +0.0, NaN and inf propagate.  A later pass sums the run sums
 * of the pass before: its rows_dev is that pass's out_dev, its stride that out_stride, with no index, no weights and
 * divisor 1.0; the passes end when every zone is one run.  Elements of a row that no entry names are never read (the elements
 * between the rows in particular); elements of out_dev beyond `runs` in a row are never written.  A wavefront owns a run, holds
 * its four entries per lane (position and weight) in registers and walks the members, the loads of four members issued before
 * the first addition; the fold goes through __shfl_down; lane 0 stores.  With few runs the members also go on the grid's
 * second dimension; which wavefront computes a (member, run) does not enter its arithmetic.  Traffic: 8 bytes per (member,
 * entry), plus 4 (index) and 8 (weights) per entry once.  Asynchronous on the device's library stream, like
 * lf_gather_rows_device; no allocation, no synchronisation, no LDS, no scratch.
 * LF_E_INVALID, with the argument named, before a device is touched: members < 1, entries or runs negative or beyond the 32-bit
 * range of a launch, runs > 0 without run_start_dev or out_dev, out_stride < runs, rows_dev NULL with entries > 0, a divisor that
 * is 0 or a NaN.  runs == 0: LF_OK, nothing is launched. */
int lf_members_zonal_device(int device, const double *rows_dev, int members, int64_t stride, double divisor, int64_t entries,
                            const int32_t *index_dev, const double *weights_dev, int64_t runs, const int32_t *run_start_dev,
                            double *out_dev, int64_t out_stride);
/* Report maps in the form a map writer takes (lf_report.hip): for up to 16 sources in ONE launch, source k < nmaps,
 * row r < rows_host[k] and cell < cells = H * W,  dst_dev[k][r * cells + cell] =
 *     idx_dev[cell] >= 0 : convert(src_dev[k][r * stride_host[k] + idx_dev[cell]] / divisor_host[k])
 *     idx_dev[cell] == -1: the fill (the cell is not land)
 *     idx_dev[cell] == -2: zero of the destination type (a land pixel the source's domain leaves out)
 * idx_dev: int32 [cells] on the device, one table for every source of the call (the caller's word that its entries stay
 * inside the rows).  The seven *_host arrays are host arrays of nmaps entries, read before the call returns.  Kinds:
 * LF_PACK_F64 sources go to LF_PACK_F64 or LF_PACK_F32 (round to nearest even, subnormal results kept, overflow to +-inf, a
 * NaN stays a NaN, -0.0 keeps its sign: numpy's astype(float32)), LF_PACK_I32 sources to LF_PACK_I32 with the fill (int32_t)fill
 * and divisor 1.  A divisor of 1.0 skips the division; any other gives the IEEE fp64 quotient.  Elements between the rows
 * of a source are never read, nothing but the rows_host[k] * cells elements of a destination is written.  A lane owns four
 * consecutive cells and stores 16 bytes at a time where the destinations allow it (16-byte aligned, rows a multiple of
 * four cells apart or a single row), one cell otherwise (LF_PACK_CELLS=1 in the environment: always; A/B switch).  Asynchronous on the stream the library calls currently go to.
 * LF_E_INVALID, with the argument named, before a device is touched: nmaps outside 1..16, cells < 0 or beyond the 32-bit
 * range of a launch, a NULL array, rows < 1, stride < 0, an unknown kind or pair of kinds, an int32 source with a divisor
 * other than 1, idx_dev or a source or destination NULL with cells > 0.  cells == 0: LF_OK, nothing is launched. */
#define LF_PACK_F64 0
#define LF_PACK_F32 1
#define LF_PACK_I32 2
int lf_pack_rasters_device(int device, int nmaps, const void *const *src_dev, void *const *dst_dev, const int32_t *rows_host,
                           const int64_t *stride_host, const int32_t *src_kind_host, const int32_t *dst_kind_host,
                           const double *divisor_host, const int32_t *idx_dev, int64_t cells, double fill);
/* host form: discharge_host[members][N] in PIXEL order updated in place, lateral_host[members][N] */
int lf_router_route_members_host(lf_router *r, double *discharge_host, const double *lateral_host,
                                 int members, int section);
/* nancheck (kinematic_wave_parallel.py:180-184): number of non-finite entries of a device vector. */
int lf_count_nonfinite(int device, const double *x_dev, int64_t n, int64_t *count);
/* launch statistics of the last route call: [0] kernel launches, [1] wide-level launches,
 * [2] narrow-run launches, [3] levels */
int lf_router_last_launches(const lf_router *r, int64_t stats[4]);
/* the schedule the last lf_routing_substeps_fused* / lf_routing_model_steps_fused call of this router took: 0 none yet,
 * 1 time-major (one launch per level through all sub-steps, plus one per level that holds a lake or reservoir), 2 the
 * skewed wavefront over level blocks, 3 the skewed wavefront over levels; -1: null router */
int lf_router_last_fused_form(const lf_router *r);
/* shape of the block plan of single router calls: [0] blocks, [1] blocks of more than one level (swept cone by cone),
 * and over those: [2] cones, [3] cone levels (one wavefront-level each: 64 lanes), [4] cells, [5] most cones in one launch.
 * [4] / (64 * [3]) = lane use of the cone sweep. */
int lf_router_route_plan_stats(const lf_router *r, int64_t out[6]);
/* the same figures for the plan a router WOULD build on a graph with blocks of up to lmax levels of at most `wide` cells
 * and cones of at most max_cone cells per level (host only: plan shapes can be studied without a device) */
int lf_graph_block_plan_stats(const lf_graph *g, int lmax, int64_t wide, int max_cone, int64_t out[6]);
/* the invariants the cone kernels rely on, checked cell by cell on the host: out[0] cells whose upstream range is not
 * inside the cone's range of the level above (must be 0), out[1] largest LDS slot + 1 a cell reads (<= max_cone),
 * out[2] largest upstream count (<= 8), out[3] cells checked */
int lf_graph_block_plan_check(const lf_graph *g, int lmax, int64_t wide, int max_cone, int64_t out[4]);
/* the order in which the fused cone kernel hands the n cones of one (block, sub-step) to its workgroups: out[i] = cone of
 * launch position i when position 0 is the workgroup with linear id first_linear_id -- the workgroups of one XCD (linear
 * id mod 8) get consecutive cones; a permutation of 0..n-1 (host only: the function the kernel calls, for the tests) */
int lf_xcd_contiguous_order(int n, unsigned int first_linear_id, int32_t *out);
/* per-kernel hipEvent profiling: when enabled every sweep launch is bracketed by an event pair.
 * lf_router_profile_read returns accumulated {launches, milliseconds, cells} per kernel class
 * (0 = prep, 1 = wide level, 2 = narrow run) since the last reset. */
int lf_router_profile_enable(lf_router *r, int on);
int lf_router_profile_read(lf_router *r, double out[9], int reset);

/* ---------------------------------------------------------------------------------------------
 * routing sub-step arithmetic (routing.py:512-603, 693-703), device vectors in pixel order
 * ------------------------------------------------------------------------------------------- */
typedef struct lf_substep_args {
    /* static [N] */
    const double *ChanLength, *InvChanLength, *ChannelAlpha, *InvChannelAlpha, *ChannelAlpha2, *InvChannelAlpha2;
    const double *Chan2M3Start, *Chan2QStart, *M3Limit, *QLimit, *PixelArea;
    const uint8_t *IsChannelKinematic;
    /* per sub-step input [N] */
    const double *SideflowChanM3;
    /* state [N], updated in place */
    double *ChanQKin, *ChanM3Kin, *Chan2QKin, *Chan2M3Kin, *CrossSection2Area, *Sideflow1Chan, *ChanQ, *sumDisDay;
    /* outputs [N] */
    double *FlowVelocity, *TravelDistance;
    /* scratch [N] x 2 */
    double *scratch0, *scratch1;
    double Beta, InvBeta, InvDtRouting, DtSec;
    int32_t split;        /* 0: single routing branch (routing.py:518-538), 1: split routing (543-604) */
    int32_t engine_order; /* 0: all vectors in pixel order, 1: all vectors in engine (sweep) order */
} lf_substep_args;
/* One routing.dynamic() sub-step: sideflow assembly, 1 or 2 router calls, volume/discharge fix-ups,
 * sumDisDay, FlowVelocity/TravelDistance.  All pointers are device memory, all in the same order
 * (pixel order, or engine order when engine_order = 1). */
int lf_routing_substep(lf_router *r, const lf_substep_args *a);
/* its three element-wise stages on their own (0: sideflow assembly, 1: main-channel fix-up + sums, 2: floodplain
 * fix-up) over n cells, for callers that run the router calls in between (lf_dist_routing_substep) */
int lf_substep_stage(int device, int stage, int64_t n, const lf_substep_args *a);
/* nsteps consecutive sub-steps as one skewed wavefront over (level, sub-step): NL + nsteps - 1 launches
 * instead of nsteps x (1..2) x NL.  Needs engine_order = 1.  a->SideflowChanM3 holds the sideflow of every
 * sub-step: sideflow_stride = 0 (one vector used by all sub-steps) or N (nsteps vectors back to back).
 * Bit-identical to nsteps calls of lf_routing_substep. */
int lf_routing_substeps_fused(lf_router *r, const lf_substep_args *a, int nsteps, int64_t sideflow_stride);
/* n_model_steps MODEL steps of steps_per_model_step sub-steps each (the loop of Lisflood_dynamic.py:179-180, model step
 * after model step) as ONE wavefront: a->SideflowChanM3 holds one sideflow vector per model step, sideflow_model_stride
 * elements apart (0: the same vector for all), a->sumDisDay is [n_model_steps][N] and zeroed by the caller (the reference
 * zeroes it at the start of every model step, Lisflood_dynamic.py:177); every other vector of `a` is the state after the
 * last model step, exactly as after n_model_steps calls of lf_routing_substeps_fused.  For callers whose channel routing
 * does not feed back into the sideflow of later steps (no structures in the loop): the land-surface part of several steps
 * first, then their channel routing in one call.  Bit-identical to the step-by-step calls. */
int lf_routing_model_steps_fused(lf_router *r, const lf_substep_args *a, int steps_per_model_step, int n_model_steps,
                                 int64_t sideflow_model_stride);
/* An ensemble through the sub-step loop: `members` (>= 1) state rows on ONE router.  `a` is one argument block: its static
 * pointers are [N] and shared by all members, its state, output and sideflow pointers are the rows of member 0; member m's
 * state and output rows sit m * member_stride elements further (member_stride >= N; elements between N and the stride are
 * neither read nor written), its sideflow m * sideflow_member_stride elements further (0: every member reads member 0's;
 * otherwise >= N with sideflow_stride = 0, >= nsteps * N with sideflow_stride = N).  Needs engine_order = 1 and a graph
 * without structure links.  Where the time-major form applies (few wide levels; LF_FUSED_TIME_MAJOR=0 / 1: never / whenever
 * possible) the members are a second grid dimension of its level kernel: one launch per level for a whole slice of members
 * (as many as the history of their router outputs has room for; LF_FUSED_MEMBERS_SLICE caps it).  Otherwise the members run
 * one after the other through the single call's schedule.  Either way every member's result is bit-identical to
 * lf_routing_substeps_fused on that member alone; lf_router_last_fused_form / lf_router_last_launches tell what ran. */
int lf_routing_substeps_fused_members(lf_router *r, const lf_substep_args *a, int nsteps, int64_t sideflow_stride,
                                      int members, int64_t member_stride, int64_t sideflow_member_stride);
/* members per slice of the time-major member form: the largest s <= min(members, 65535, cap if cap > 0) with
 * s * nsteps * n * 8 * (split ? 2 : 1) <= budget_bytes; 0 when not even one member fits (host only) */
int64_t lf_fused_members_slice(int members, int64_t n, int nsteps, int split, int64_t budget_bytes, int cap);

/* ---------------------------------------------------------------------------------------------
 * LDD one-hop upstream reduction == np.bincount(downstruct, weights)[:N] (routing.py:159-164,
 * lakes.py:215, reservoir.py:190) and upstream(ldd, x) (routing.py:387)
 * ------------------------------------------------------------------------------------------- */
int lf_upstream_sum_device(lf_router *r, const double *w_dev, double *out_dev);
int lf_upstream_sum_host(lf_router *r, const double *w_host, double *out_host);
/* the same reduction directly on H x W rasters (uint8 LDD codes, 0 = sea / missing; fp64 weights, device memory):
 * LDS-staged 3 x 3 neighbourhoods, coalesced rows, neighbours added in ascending source index. */
int lf_upstream_sum_raster_device(int device, const uint8_t *ldd_raster_dev, const double *w_raster_dev,
                                  double *out_raster_dev, int H, int W);
/* accuflux(ldd, x): sum of x over all upstream cells including the cell itself (routing.py:98) */
int lf_accuflux_host(lf_router *r, const double *x_host, double *out_host);

/* accuflux on engine-order device vectors (acc_ord[p] = x_ord[p] + sum over the upstream cells) */
int lf_accuflux_ordered_device(lf_router *r, const double *x_ord_dev, double *acc_ord_dev);

/* ---------------------------------------------------------------------------------------------
 * LDD operations of routing.initial / structures.initial (routing.py:90-171, structures.py:44-61; the reference calls
 * PCRaster 4.3.3: lddrepair, lddmask, downstream, catchment) and the per-catchment totals of routing.dynamic's
 * mass-balance bookkeeping (routing.py:483-499, 645-691).  Rasters are H x W uint8 keypad codes, 0 = missing value.
 * ------------------------------------------------------------------------------------------- */
/* lddrepair: cells draining off the map or into a missing value become pits (routing.py:125) */
int lf_lddrepair_raster_device(int device, const uint8_t *ldd_dev, uint8_t *out_dev, int H, int W);
/* lddmask(ldd, keep): cells outside keep become missing values, cells draining out of keep become pits (:90, :118) */
int lf_lddmask_raster_device(int device, const uint8_t *ldd_dev, const uint8_t *keep_dev, uint8_t *out_dev, int H, int W);
/* host-buffer form of both: keep_host = NULL -> lddrepair, else lddmask */
int lf_ldd_raster_host(int device, const uint8_t *ldd_host, const uint8_t *keep_host, uint8_t *out_host, int H, int W);
/* downstream(ldd, x): value of x at the downstream cell, pits keep their own (routing.py:141, 162; structures.py:51) */
int lf_downstream_device(lf_router *r, const double *x_pix_dev, double *out_pix_dev);
int lf_downstream_host(lf_router *r, const double *x_host, double *out_host);
/* catchment(ldd, points): id of the first non-zero point met going downstream (a point cell belongs to its own
 * catchment), 0 if none (routing.py:168-171).  Pointer jumping over the downstream links: O(log depth) passes. */
int lf_catchments_device(lf_router *r, const int32_t *points_pix_dev, int32_t *labels_pix_dev);
int lf_catchments(lf_router *r, const int64_t *points_host, int64_t *labels_host);
/* np.take(np.bincount(Catchments, weights=w), Catchments) for Catchments = catchment(ldd, pit(ldd)): every cell gets
 * the total of w over its whole tree (routing.py:483-499, 645-691; equal to rounding, the summation order differs) */
/* (synchronous: the totals are complete when it returns; the asynchronous form is the multi-vector one below) */
int lf_catchment_totals_device(lf_router *r, const double *w_pix_dev, double *out_pix_dev);
int lf_catchment_totals_host(lf_router *r, const double *w_host, double *out_host);
/* nv (<= 4) weight vectors in ONE sweep (the mass-balance terms of routing.py:645-691 come several at a time): the
 * device form is asynchronous on the library stream and, after a router's first call (which finds every cell's outlet
 * once, by pointer jumping), neither allocates nor synchronises; the host form takes nv vectors of N doubles back to
 * back.  accuflux runs on the router's block plan (blocks of levels cone by cone), like a router call. */
int lf_catchment_totals_multi_device(lf_router *r, int nv, const double *const *w_pix_dev, double *const *out_pix_dev);
int lf_catchment_totals_multi_host(lf_router *r, int nv, const double *w_host, double *out_host);
int lf_accuflux_ordered_multi_device(lf_router *r, int nv, const double *const *x_ord_dev, double *const *acc_ord_dev);

/* ---------------------------------------------------------------------------------------------
 * soil: replaces interception_water_balance (soilloop.py:27-70) and soilColumnsWaterBalance
 * (soilloop.py:78-355).  Layouts as in the reference: [V,N] / [L,N] C-order fp64, bool arrays 1 byte.
 * ------------------------------------------------------------------------------------------- */
typedef struct lf_interception_args {
    double *Interception, *TaInterception, *LeafDrainage, *CumInterception; /* [V,N] in/out */
    const double *LAI;               /* [V,N] */
    const double *Rain;              /* [N]   */
    const double *TaInterceptionMax; /* [V,N] */
    double drainageK;
    int64_t V, N;
} lf_interception_args;

/* The seven diagnostics Theta1a, Theta1b, Theta2, Sat1a, Sat1b, Sat1, Sat2 (soilloop.py:330-336) are OPTIONAL in the
 * device forms: a NULL pointer = not reported, not computed (nothing else in the column's water balance reads them). */
typedef struct lf_soil_args {
    /* [L,N] statics */
    const uint8_t *PoreSpaceNotZero1a, *PoreSpaceNotZero1b, *PoreSpaceNotZero2;
    const double *KSat1a, *KSat1b, *KSat2, *GenuInvM1a, *GenuInvM1b, *GenuInvM2, *GenuM1a, *GenuM1b, *GenuM2;
    const double *WRes1a, *WRes1b, *WRes1, *WRes2, *WWP1a, *WWP1b, *WWP1, *WWP2, *WFC1a, *WFC1b, *WFC1, *WFC2;
    const double *SoilDepth1a, *SoilDepth1b, *SoilDepth2, *WS1a, *WS1b, *WS1, *WS2, *StoreMaxPervious;
    /* [N] */
    const double *Rain, *SnowMelt, *b_Xinanjiang, *PowerInfPot, *PowerPrefFlow, *UpperZoneK, *GwPercStep;
    const uint8_t *isFrozenSoil;
    /* [V,N] in */
    const double *LeafDrainage, *Interception, *ESMax;
    /* [V,N] in/out and out */
    double *AvailableWaterForInfiltration, *DSLR, *ESAct, *PrefFlow, *Infiltration, *W1a, *W1b, *W1, *W2;
    double *Theta1a, *Theta1b, *Theta2, *Sat1a, *Sat1b, *Sat1, *Sat2, *SeepTopToSubA, *SeepTopToSubB, *SeepSubToGW;
    double *UZOutflow, *UZ, *GwPercUZLZ;
    /* small, ALWAYS host memory */
    const int64_t *index_landuse_all; /* [V] */
    const uint8_t *is_irrigated;      /* [V] */
    const uint8_t *is_paddy_irrig;    /* [V] */
    /* [n_paddy, N]; host memory in lf_soil_columns_host, device memory in lf_soil_columns_device;
     * paddy_any[n_paddy] (host) tells the device form which rows have any inactive pixel */
    const uint8_t *paddy_inactive;
    const uint8_t *paddy_any;
    double DtDay, AvWaterThreshold, CourantCrit, DrainedFraction;
    int64_t V, L, N;
} lf_soil_args;

/* dynamic_canopy (soilloop.py:519-627) for the three prescribed vegetation fractions: TaInterceptionMax,
 * interception kernel, potential transpiration, water-stress reduction, abstraction of transpiration from
 * layers 1a/1b.  [V,N] / [L,N] C-order; index_landuse[V] (host) maps each vegetation row to its land-use row
 * (the reference indexes W1/W1a/W1b by the land-use row there, soilloop.py:592-627 -- reproduced). */
typedef struct lf_canopy_args {
    /* [V,N] in/out */
    double *Interception, *TaInterception, *LeafDrainage, *CumInterception;
    double *potential_transpiration, *RWS, *Ta;
    double *W1a, *W1b, *W1;
    /* [V,N] in */
    const double *LAI, *LAITerm;
    /* [L,N] in */
    const double *CropCoef, *CropGroupNumber, *WFC1, *WFC1a, *WFC1b, *WWP1, *WWP1a, *WWP1b;
    /* [N] in */
    const double *Rain, *EWRef, *ETRef;
    const uint8_t *isFrozenSoil;
    const int64_t *index_landuse; /* [V], host */
    double LeafDrainageK, DtDay, InvDtDay;
    int64_t V, L, N;
    /* option branches of the method, each switched on by a non-NULL output:
     *   repStressDays (soilloop.py:597-598): SoilMoistureStressDays[V,N] = DtDay where RWS < 1, else 0
     *   wateruse      (soilloop.py:582-587): WFilla[N] / WFillb[N] = min(WCrit1a / WCrit1b, WPF3a / WPF3b) of the land-use
     *                 row of vegetation row `irrigated_veg` (the "Irrigated" fraction; < 0: none); WPF3a / WPF3b [L,N] */
    double *SoilMoistureStressDays;
    double *WFilla, *WFillb;
    const double *WPF3a, *WPF3b;
    int64_t irrigated_veg;
} lf_canopy_args;
int lf_canopy_device(int device, const lf_canopy_args *a);
/* The land surface of a model step in ONE pass over the columns: dynamic_canopy (soilloop.py:519-627), ESMax = ESRef *
 * LAITerm (:638) and soilColumnsWaterBalance (:78-355) -- the lane that runs a column's canopy carries LeafDrainage,
 * Interception, W1a / W1b / W1 and ESMax into the column's soil water balance in registers (Lisflood_dynamic.py:114-123
 * calls the two methods back to back; nothing reads the vectors in between).  Bit-identical to lf_canopy_device +
 * lf_scale_rows_device + lf_soil_columns_device (derived != 0: _derived).  `canopy` and `soil` must describe the same
 * columns: V = L, same N, index_landuse[v] == v in both, no paddy fraction, and the vectors both structs name (W1a, W1b,
 * W1, Interception, LeafDrainage, Rain, isFrozenSoil, WWP1a/b, WFC1a/b) must be the same device vectors -- LF_E_INVALID
 * otherwise (use the separate entry points then).  soil->ESMax is not read; ESRef_dev is the [N] vector. */
int lf_land_columns_device(int device, const lf_canopy_args *canopy, const lf_soil_args *soil, const double *ESRef_dev,
                           int derived);
/* The soil columns / the land surface of an ENSEMBLE -- members that share the LDD, the geometry and the parameters -- in
 * one call.  The convention of lf_routing_substeps_fused_members: the argument blocks are those of the single calls and
 * their per-member pointers name member 0.
 *   per member, m * member_stride elements further on (member_stride >= V*N; the elements between are neither read nor
 *     written): every vector the single call writes, LeafDrainage / Interception / ESMax of the soil block, the ten in/out
 *     rows of the canopy block, SoilMoistureStressDays, WFilla and WFillb when given
 *   per-member forcing, m * forcing_member_stride elements further on (0: every member reads member 0's, otherwise >= N):
 *     Rain, SnowMelt, isFrozenSoil (bytes), EWRef, ETRef, ESRef
 *   shared: every [L,N] array, the five [N] calibration vectors (b_Xinanjiang, PowerInfPot, PowerPrefFlow, UpperZoneK,
 *     GwPercStep), LAI, LAITerm, WPF3a / WPF3b, paddy_inactive
 * A NULL diagnostic pointer (Theta*, Sat*) means "not reported" for every member.  The checks of the single calls apply
 * unchanged; members < 1, member_stride < V*N, 0 < forcing_member_stride < N and members * tiles (256 columns each) beyond
 * the 32-bit range are refused with LF_E_INVALID before any device is touched.  The unit of work is (tile, member): ONE
 * launch of the column kernel covers all of them, tile-major, dealt to the workgroups so that the members of a tile run next
 * to each other on one XCD (lf_land_members_unit), and one launch of the straggler kernel runs behind it; the statics of a
 * tile are then streamed from HBM once per tile, not once per member.  Every member's result is bit-identical to the single
 * call on that member alone; members == 1 IS the single call.  LF_LAND_MEMBERS=0: the members one after the other through
 * the single call (the same bits).  The workspace grows to members times the single call's; afterwards
 * lf_soil_last_deferred and lf_soil_substep_histogram cover all members (the sums of the members' own). */
int lf_soil_columns_members_device(int device, const lf_soil_args *a, int derived, int members, int64_t member_stride,
                                   int64_t forcing_member_stride);
int lf_land_columns_members_device(int device, const lf_canopy_args *canopy, const lf_soil_args *soil,
                                   const double *ESRef_dev, int derived, int members, int64_t member_stride,
                                   int64_t forcing_member_stride);
/* the form the last soil / land-surface call on the device took: 0 none yet, 1 single call, 2 members in one launch,
 * 3 member after member */
int lf_soil_last_form(int device);
/* (tile, member) of launch position `position` of the member launch over ntiles * members units, when the workgroup at
 * position 0 has linear id 0: the workgroups of one XCD (linear id mod 8) get a run of consecutive units of the tile-major
 * order tile * members + member (host only: the function the kernel calls, for the tests) */
int lf_land_members_unit(int64_t ntiles, int members, int64_t position, int64_t *tile, int *member);

/* suctionUnsaturatedSoilPF + pressureHead (soilloop.py:427-432, 673-695; option simulatePF): pF = log10 of the capillary
 * head of the three soil layers, -1 where the head is not positive.  [V,N] by vegetation row, [L,N] by land-use row. */
typedef struct lf_soil_pf_args {
    double *pF0, *pF1, *pF2;                 /* [V,N] out */
    const double *W1a, *W1b, *W2;            /* [V,N] */
    const double *WRes1a, *WRes1b, *WRes2, *WS1a, *WS1b, *WS2; /* [L,N] */
    const uint8_t *PoreSpaceNotZero1a, *PoreSpaceNotZero1b, *PoreSpaceNotZero2;
    const double *GenuInvAlpha1a, *GenuInvAlpha1b, *GenuInvAlpha2, *GenuInvM1a, *GenuInvM1b, *GenuInvM2, *GenuInvN1a,
        *GenuInvN1b, *GenuInvN2;             /* [L,N] */
    const int64_t *index_landuse_all;        /* [V], host */
    double HeadMax;
    int64_t V, L, N;
} lf_soil_pf_args;
int lf_soil_pf_device(int device, const lf_soil_pf_args *a);
/* out[v,p] = row[p] * m[v,p]  (ESMax = ESRef * LAITerm, soilloop.py:638) */
int lf_scale_rows_device(int device, const double *row_dev, const double *m_dev, double *out_dev, int64_t V, int64_t N);

/* surface_routing.dynamic (surface_routing.py:115-212), prescribed fractions (V = L = 3, rows Rainfed /
 * Forest / Irrigated), all vectors device memory in pixel order.  Three routers share one graph. */
typedef struct lf_surface_args {
    /* [3,N] in */
    const double *SoilFraction, *AvailableWaterForInfiltration, *Infiltration, *OFAlpha; /* OFAlpha rows: Other, Forest, Direct */
    /* [N] in */
    const double *DirectRunoff, *UZOutflowPixel, *LZOutflowToChannelPixel;
    const uint8_t *IsChannel;
    /* [N] state, in/out */
    double *OFQDirect, *OFQOther, *OFQForest;
    /* [N] out */
    double *OFM3Direct, *OFM3Other, *OFM3Forest, *SurfaceRunoff, *TotalRunoff, *OFToChanM3, *WaterDepth, *ToChanM3Runoff,
        *ToChanM3RunoffDt;
    double *SurfaceRunSoil; /* [3,N] out */
    double *scratch;        /* [3,N] */
    double Beta, MMtoM3, M3toMM, PixelLength, InvPixelLength, DtSec, InvDtSec, InvNoRoutSteps;
    int64_t N;
} lf_surface_args;
int lf_surface_step(lf_router *direct_router, lf_router *other_router, lf_router *forest_router,
                    const lf_surface_args *a);
/* The same with EVERY vector of `a` in the sweep (engine) order of the three routers' shared graph instead of pixel order:
 * the element-wise parts do not care, and the routers then stream their vectors (lf_router_route_ordered: ~54 B per cell
 * instead of ~135 through the position -> pixel table).  A caller that keeps a whole model step resident permutes its
 * per-pixel fields once (lf_graph_layout gives the table) -- lisflood_amd.hotpath.HotPathDevice does. */
int lf_surface_step_ordered(lf_router *direct_router, lf_router *other_router, lf_router *forest_router,
                            const lf_surface_args *a);
/* lf_surface_step_ordered for an ENSEMBLE, in the convention of lf_land_columns_members_device: `a` is the block of the
 * single call and names member 0's rows, every vector in the sweep order of the routers' graph.
 *   shared: SoilFraction, OFAlpha, IsChannel
 *   per member, m * member_stride elements further on (member_stride >= 3 * N): AvailableWaterForInfiltration, Infiltration,
 *     SurfaceRunSoil
 *   per member, m * pixel_member_stride elements further on (pixel_member_stride >= N): every other [N] vector
 *   scratch: 3 * members * pixel_member_stride elements, laid out [3][members][pixel_member_stride] by the call -- the three
 *     lateral-inflow row sets then have the stride of the discharge rows
 * Elements between rows are neither read nor written.  The two element-wise kernels run once for all (block of 256 pixels,
 * member) units, block-major and dealt to the workgroups as lf_land_members_unit says; between them ONE
 * lf_router_route_ordered_members_multi call sweeps the three routers.  Every member's result is bit-identical to
 * lf_surface_step_ordered on that member alone; members == 1 IS that call.  LF_SURFACE_MEMBERS=0, read per call: member
 * after member through the single call (the same bits).  members < 1, a stride too small and members * blocks beyond the
 * 32-bit range are refused with LF_E_INVALID before a device is touched. */
int lf_surface_step_members(lf_router *direct_router, lf_router *other_router, lf_router *forest_router,
                            const lf_surface_args *a, int members, int64_t member_stride, int64_t pixel_member_stride);
/* the form the last pixel-aggregates (stage 0) / surface-step (stage 1) call on the device took: 0 none yet, 1 single call,
 * 2 members in one launch, 3 member after member (as lf_soil_last_form) */
int lf_module_last_form(int device, int stage);
/* (pixel block, member) of launch position `position` of the element-wise member kernels (the per-pixel aggregates and the two
 * kernels of the overland step) over nblocks * members units, when the workgroup at position 0 has linear id 0: the order of
 * lf_land_members_unit (host only: the function the kernels call, for the tests) */
int lf_module_members_unit(int64_t nblocks, int members, int64_t position, int64_t *block, int *member);

/* In-loop structures of routing.dynamic (routing.py:441-478): lakes (lakes.py:199-297, Modified Puls), reservoirs
 * (reservoir.py:173-322), inflow hydrographs (inflow.py:129-147), transmission loss (transmission.py:67-89) and
 * the SideflowChanM3 assembly (routing.py:462-478), all on device vectors in ONE order (pixel or engine).
 * Sites are few (LF_ETRS89: 5 lakes, 64 reservoirs): one lane per site; per-site inflow = sum of ChanQ over
 * site_ups_idx[site_ups_ptr[i] .. site_ups_ptr[i+1]) in ascending pixel id (np.bincount(downstruct, ChanQ)).
 * Any pointer group may be NULL / its count 0 (option switched off). */
typedef struct lf_inloop_args {
    const double *ChanQ; /* [N] discharge at the start of the sub-step */
    /* lakes [n_lakes] */
    int64_t n_lakes;
    const int32_t *lake_cell, *lake_ups_ptr, *lake_ups_idx;
    const double *LakeFactor, *LakeFactorSqr, *LakeAreaCC;
    double *LakeStorageM3CC, *LakeInflowOldCC, *LakeOutflowCC, *LakeStorageM3BalanceCC, *LakeLevelCC, *LakeInflowCC;
    double *QLakeOutM3Dt; /* [N], written at the lake cells only */
    /* reservoirs [n_res] */
    int64_t n_res;
    const int32_t *res_cell, *res_ups_ptr, *res_ups_idx;
    const double *TotalReservoirStorageM3CC, *MinReservoirOutflowCC, *NormalReservoirOutflowCC,
        *NonDamagingReservoirOutflowCC, *ConservativeStorageLimitCC, *NormalStorageLimitCC, *FloodStorageLimitCC,
        *Normal_FloodStorageLimitCC, *DeltaO, *DeltaLN, *DeltaNFL;
    double *ReservoirStorageM3CC, *ReservoirFillCC, *ReservoirInflowCC;
    double *QResOutM3Dt; /* [N], written at the reservoir cells only */
    /* inflow hydrographs [N] (NULL = option off) */
    const double *QInM3Old, *QDelta;
    double *QInDt, *QinADDEDM3;
    /* transmission loss [N] (NULL = option off) */
    const uint8_t *UpTrans;
    double *TransLossM3Dt, *TransCum;
    double TransPower1, TransPower2, TransSub;
    /* sideflow assembly [N]: out = ToChanM3RunoffDt - EvaAddM3Dt - WUseAddM3Dt + QInDt - TransLossM3Dt
     *                              + QLakeOutM3Dt + QResOutM3Dt - ChannelToPolderM3Dt   (NULL terms skipped) */
    const double *ToChanM3RunoffDt, *EvaAddM3Dt, *WUseAddM3Dt, *ChannelToPolderM3Dt;
    double *SideflowChanM3;
    double DtRouting, InvNoRoutSteps;
    int64_t N;
    int32_t step; /* NoRoutingExecuted */
} lf_inloop_args;
int lf_inloop_structures(int device, const lf_inloop_args *a);
/* The whole loop `for s in range(NoRoutSteps): lakes/reservoir/inflow/transmission.dynamic_inloop(s);
 * routing.dynamic(s)` (Lisflood_dynamic.py:179-180 with routing.py:441-478) as ONE skewed wavefront: the cell kernel
 * of lf_routing_substeps_fused assembles SideflowChanM3 itself (inflow hydrographs, transmission loss, the
 * structures' outflow) and a one-lane-per-site kernel runs each lake / reservoir for sub-step s = t - level(site)
 * right before launch t.  Needs: engine_order = 1 everywhere (`in` holds engine-order vectors and site lists in
 * engine positions, `in->step` is ignored), and a router whose graph was built by lf_graph_create_ex with the
 * uncut links of the structures (every cell feeding a site on the site's level; checked once per set of device
 * site lists, whose contents must not change afterwards).  Bit-identical to the
 * sub-step-by-sub-step sequence lf_inloop_structures + lf_routing_substep.
 * On graphs of few wide levels (the rule of lf_routing_substeps_fused; LF_FUSED_TIME_MAJOR=0 / 1: never / whenever it
 * applies) the call takes the TIME-MAJOR form instead: level after level, every cell through all its sub-steps with its
 * state -- and the inflow hydrograph, transmission loss and sideflow terms -- in registers.  The cells feeding a site write
 * their ChanQ of every sub-step to a small [nsteps + 1][feeders] buffer; the site cells of a level run in a launch of
 * their own behind the level's (one lane per site: the site's update, then the cell's sub-step, sub-step after sub-step).
 * It needs the site plan to apply (lf_site_plan: no chained sites, no shared cells) and room for the [nsteps][N]
 * history; otherwise the skewed wavefront runs.  Same bits either way; lf_router_last_fused_form tells which ran. */
int lf_routing_substeps_fused_structures(lf_router *r, const lf_substep_args *a, const lf_inloop_args *in, int nsteps);
/* An ensemble through that loop: `members` (>= 1) members on ONE router, with the lakes, reservoirs, inflow hydrographs and
 * transmission loss of each inside the call.  `a` and `in` are member 0's blocks.  Shared by all members: every static of
 * `a`, the site lists and site parameters of `in` (lake_cell .. LakeAreaCC, res_cell .. DeltaNFL), UpTrans and the scalars.
 * Per member, m strides further than member 0's:
 *   member_stride (>= N): the state and output rows of `a` and the dense [N] rows of `in` (QLakeOutM3Dt, QResOutM3Dt, QInDt,
 *     QinADDEDM3, TransLossM3Dt, TransCum, SideflowChanM3; in->ChanQ is a->ChanQ);
 *   lake_member_stride (>= n_lakes) / res_member_stride (>= n_res): the six lake / three reservoir state vectors (ignored
 *     when the count is 0);
 *   forcing_member_stride (0: every member reads member 0's, else >= N): ToChanM3RunoffDt, EvaAddM3Dt, WUseAddM3Dt,
 *     ChannelToPolderM3Dt, QInM3Old, QDelta.
 * Elements between a row's length and its stride are neither read nor written; a NULL pointer (option off) is NULL for every
 * member.  members < 1, a negative or too small stride, a forcing stride strictly between 0 and N, null blocks and
 * nsteps < 1 are refused with LF_E_INVALID and a message naming the argument, before any device is touched; a refused call
 * advances nothing.  Where the time-major form applies to the ensemble (the site plan applies or there is no site, nsteps > 1,
 * the width rule of lf_routing_substeps_fused with the lanes counted over the members; LF_FUSED_TIME_MAJOR=0 / 1: never /
 * whenever possible) the members go slice by slice (lf_fused_members_slice over the history budget, LF_FUSED_MEMBERS_SLICE
 * caps it): one launch per level for the cells of the whole slice and one more behind it on a level that holds sites, each
 * member with a [nsteps + 1][feeders] buffer of its own.  Otherwise (chained sites, deep graphs, one sub-step, no room) the
 * members run one after the other through the single call's schedule, the site checks and flag passes once.  Either way
 * every member's result is bit-identical to lf_routing_substeps_fused_structures on that member alone; members = 1 IS that
 * call.  lf_router_last_fused_form / lf_router_last_launches tell what ran (launches summed over slices or members). */
int lf_routing_substeps_fused_structures_members(lf_router *r, const lf_substep_args *a, const lf_inloop_args *in,
                                                 int nsteps, int members, int64_t member_stride, int64_t lake_member_stride,
                                                 int64_t res_member_stride, int64_t forcing_member_stride);
/* drops the cached validation of the site lists (call after rebuilding lake_cell / lake_ups_idx / res_cell /
 * res_ups_idx, even if the new lists live at the old addresses) */
int lf_router_reset_site_cache(lf_router *r);

/* The per-pixel aggregates between the soil columns and surface routing, one pass:
 * opensealed.dynamic (opensealed.py:40-71), soil.dynamic_perpixel (soil.py:471-514; deffraction =
 * sum over the fractions of SoilFraction * X, Lisflood_initial.py:69-71,393-396) and groundwater.dynamic
 * (groundwater.py:134-180).  Prescribed fractions (V = L = 3, fraction v uses land-use row v). */
/* Every output but DirectRunoff, UZOutflowPixel, LZOutflowToChannelPixel and the states CumInterSealed / LZ is OPTIONAL:
 * a NULL pointer means the map is not reported -- it is not computed, and a [3,N] input only it reads may be NULL too
 * (the reference computes all of them every step and writes the ones its rep* options name). */
typedef struct lf_pixel_args {
    /* [3,N] in */
    const double *SoilFraction, *TaInterception, *Ta, *ESAct, *PrefFlow, *Infiltration, *SeepTopToSubA, *SeepTopToSubB,
        *SeepSubToGW, *Theta1a, *Theta1b, *Theta2, *W1a, *W1b, *W2, *UZOutflow, *GwPercUZLZ, *SoilDepthTotal;
    /* [N] in */
    const double *Rain, *SnowMelt, *EWRef, *SMaxSealed, *DirectRunoffFraction, *WaterFraction, *LowerZoneK, *LZThreshold,
        *GwLossStep;
    /* [N] state in/out */
    double *CumInterSealed, *LZ, *LZInflowCUM, *TaInterceptionCUM, *TaCUM, *ESActCUM, *GwLossCUM;
    /* [N] out */
    double *RainSnowmelt, *EWaterAct, *InterSealed, *TASealed, *DirectRunoff, *TaInterceptionAll, *TaPixel, *ESActPixel,
        *PrefFlowPixel, *InfiltrationPixel, *ThetaAll, *SeepTopToSubPixelA, *SeepTopToSubPixelB, *SeepSubToGWPixel,
        *Theta1aPixel, *Theta1bPixel, *Theta2Pixel, *LZOutflow, *UZOutflowPixel, *GwPercUZLZPixel, *GwLossLZ, *LZAvInflow,
        *LZOutflowToChannelPixel;
    double *Theta; /* [3,N] out */
    double InvDtDay, TimeSinceStart;
    int64_t N;
} lf_pixel_args;
int lf_pixel_aggregates_device(int device, const lf_pixel_args *a);
/* The per-pixel aggregates of an ENSEMBLE in one launch, in the convention of lf_land_columns_members_device: `a` is the
 * block of the single call and names member 0's rows.
 *   shared: SoilFraction, SoilDepthTotal, SMaxSealed, DirectRunoffFraction, WaterFraction, LowerZoneK, LZThreshold, GwLossStep
 *   per member, m * member_stride elements further on (member_stride >= 3 * N, the land ensemble's stride): every other [3,N]
 *     input, and Theta
 *   per member, m * pixel_member_stride elements further on (pixel_member_stride >= N): every [N] state and output
 *   forcing, m * forcing_member_stride elements further on (0: shared, otherwise >= N): Rain, SnowMelt, EWRef
 * Elements between rows are neither read nor written; NULL (not reported) maps work as in the single call, for every member.
 * The unit of work is (block of 256 pixels, member): one launch covers all units, block-major and dealt to the workgroups as
 * lf_land_members_unit says, so the members of a block run next to each other on one XCD whose L2 holds the block's 13
 * static values per pixel.  Every member's result is bit-identical to the single call on that member alone; members == 1 IS
 * the single call.  LF_PIXEL_MEMBERS=0, read per call: member after member through the single kernel (the same bits).
 * The checks of the single call apply; members < 1, a stride too small, 0 < forcing_member_stride < N and members * blocks
 * beyond the 32-bit range are refused with LF_E_INVALID before a device is touched. */
int lf_pixel_aggregates_members_device(int device, const lf_pixel_args *a, int members, int64_t member_stride,
                                       int64_t pixel_member_stride, int64_t forcing_member_stride);

/* The front of the model step: snow.dynamic followed by frost.dynamic, three elevation zones (0: the highest).  From
 * precipitation and average temperature it makes the Rain, SnowMelt and isFrozenSoil the land surface starts from, and it
 * carries the snow pack of the zones (SnowCoverS) and the frost index from one step to the next.  All arithmetic is fp64,
 * every + - * / one IEEE operation in the order written, max / min are numpy's maximum / minimum (a NaN operand gives
 * NaN), comparisons are false on NaN; exp is OCML's (exactly 1 where its argument is a zero).  Per pixel p:
 *   seas = SnowSeasonTerm + SnowMeltCoef[p];  Snow = Rain = SnowMelt = SnowCover = 0
 *   for i in 0, 1, 2:
 *     TavgS = Tavg + DeltaTSnow[p] * (i - 1)                       ((i - 1) as the doubles -1.0, 0.0, 1.0)
 *     SnowS = TavgS <  TempSnow ? SnowFactor[p] * Precipitation : 0
 *     RainS = TavgS >= TempSnow ? Precipitation : 0
 *     MeltS = max((TavgS - TempMelt) * seas * (1 + 0.01 * RainS) * DtDay, 0)
 *     IceS  = max((i < 2 ? Tavg : TavgS) * IceMeltCoef * DtDay * SummerSeason, 0)
 *     MeltS = max(min(MeltS + IceS, SnowCoverS[i]), 0)
 *     SnowCoverS[i] = SnowCoverS[i] + SnowS - MeltS
 *     Snow += SnowS;  Rain += RainS;  SnowMelt += MeltS;  SnowCover += SnowCoverS[i]
 *   Snow /= 3;  Rain /= 3;  SnowMelt /= 3;  SnowCover /= 3          (divisions)
 *   Kfrost = Tavg < 0 ? 0.08 : 0.5
 *   rate = -(1 - Afrost) * FrostIndex - Tavg * exp(-0.04 * Kfrost * SnowCover / SnowWaterEquivalent)
 *   FrostIndex = max(FrostIndex + rate * DtDay, 0);  isFrozenSoil = FrostIndex > FrostIndexThreshold
 * SnowSeasonTerm and SummerSeason are the step's season values, taken as given (lisflood_amd.snow_frost.season_terms). */
typedef struct lf_snow_frost_args {
    const double *Precipitation, *Tavg;                   /* rows, forcing layout */
    double *SnowCoverS;                                   /* [3,N] rows, in / out */
    double *FrostIndex;                                   /* [N] rows, in / out */
    double *Rain, *SnowMelt, *Snow, *SnowCover;           /* [N] rows, out; Snow may be NULL */
    uint8_t *isFrozenSoil;                                /* byte rows, out */
    const double *DeltaTSnow, *SnowMeltCoef, *SnowFactor; /* [N], shared by all members */
    double TempSnow, TempMelt, IceMeltCoef, DtDay, Afrost, SnowWaterEquivalent, FrostIndexThreshold, SnowSeasonTerm,
        SummerSeason;
    int64_t N;
} lf_snow_frost_args;
/* One kernel and one enqueue for a single run (members = 1) and an ensemble: `a` names member 0's rows, member m's lie
 * m * zone_stride elements further on (SnowCoverS, zone i at i * N inside), m * row_stride elements further on (FrostIndex
 * and the [N] outputs; isFrozenSoil: row_stride BYTES) and m * forcing_stride elements further on (Precipitation, Tavg;
 * 0: one row for all).  Elements between a row's length and its stride are neither read nor written.  A lane owns a pixel
 * and walks up to 8 members: the statics are read once per pixel and slice of 8 members.
 * Halves: FrostIndex == NULL (and then isFrozenSoil == NULL): snow only.  SnowCoverS == NULL: frost only, SnowCover is
 * then an INPUT and Precipitation, Rain, SnowMelt, Snow and the three statics are not used (the first four must be NULL).
 * Refused with LF_E_INVALID before anything is enqueued: every other NULL combination, two vectors of which one is
 * written sharing an element, N < 0, members < 1, zone_stride < 3 * N, row_stride < N, forcing_stride neither 0 nor at
 * least N.  N == 0 succeeds and launches nothing.  Enqueued on the current stream (it follows lf_side_stream_begin); the
 * call does not synchronise. */
int lf_snow_frost_members_device(int device, const lf_snow_frost_args *a, int members, int64_t zone_stride, int64_t row_stride,
                                 int64_t forcing_stride);

/* host-buffer forms (drop-in for the numba kernels; PCIe-inclusive) */
int lf_interception_host(int device, const lf_interception_args *a);
int lf_soil_columns_host(int device, const lf_soil_args *a);
/* device-resident forms: every array pointer is device memory (except the small per-vegetation ones).  The soil call keeps a
 * per-device workspace for the columns that leave their tile (above LF_SOIL_TRIP_CAP = 6 Courant sub-steps, up to 48 per
 * tile of 256 columns): ~15.4 KB per tile = ~60 bytes per column, grow-only, released by lf_device_trim. */
int lf_interception_device(int device, const lf_interception_args *a);
int lf_soil_columns_device(int device, const lf_soil_args *a);
/* The same for a caller that vouches for the relations soil.py:180-228 establishes between its parameter arrays (GenuInvM =
 * 1 / GenuM; WS1 = WS1a + WS1b, and so WRes1, WFC1, WWP1; PoreSpaceNotZero = SoilDepth != 0 and WS != 0): those ten arrays
 * are recomputed (one IEEE operation each: the same bits) instead of read and may be NULL -- 59 bytes less per column. */
int lf_soil_columns_device_derived(int device, const lf_soil_args *a);
/* instrumentation: columns of the last lf_soil_columns_device call that needed > 1 Courant sub-step */
int lf_soil_last_deferred(int device, int64_t *count);
/* ... and their histogram by trip count (hist[k] = columns with k sub-steps, last bin = nbins-1 or more; the engine
 * keeps counts up to 127) */
int lf_soil_substep_histogram(int device, int64_t *hist, int nbins);

/* ---------------------------------------------------------------------------------------------
 * multi-GPU: the raster is split into contiguous row blocks, one rank (process, GPU) per block; boundary
 * discharge is exchanged with RCCL Send/Recv between vertical neighbours.  The reference has no
 * distributed code; the result is bit-identical to the single-domain call (see csrc/lf_dist.hip).
 * Setup protocol (host side, any transport for the tiny phase vectors):
 *   1. lf_dist_graph_create with the rank's own rows and the one halo row above / below (NULL at the
 *      raster's edge);
 *   2. repeat { get_export_phases -> swap with the neighbours -> set_ghost_phases } until no rank changes;
 *   3. lf_dist_graph_finalize(max over ranks of lf_dist_graph_local_num_phases).
 * ------------------------------------------------------------------------------------------- */
int lf_dist_graph_create(const uint8_t *ldd_local, const uint8_t *mask_local, int H_local, int W,
                         const uint8_t *ldd_top, const uint8_t *mask_top, const uint8_t *ldd_bottom,
                         const uint8_t *mask_bottom, lf_dist_graph **out);
void lf_dist_graph_destroy(lf_dist_graph *g);
int64_t lf_dist_graph_num_pixels(const lf_dist_graph *g);
int lf_dist_graph_counts(const lf_dist_graph *g, int64_t out[4]); /* exports top,bottom; ghosts top,bottom */
int lf_dist_graph_get_export_phases(const lf_dist_graph *g, int32_t *top, int32_t *bottom);
int lf_dist_graph_set_ghost_phases(lf_dist_graph *g, const int32_t *top, const int32_t *bottom, int *changed);
int lf_dist_graph_local_num_phases(const lf_dist_graph *g);
int lf_dist_graph_finalize(lf_dist_graph *g, int nphases);
int64_t lf_dist_graph_state_size(const lf_dist_graph *g); /* N local cells + ghost slots */
int lf_dist_graph_num_phases(const lf_dist_graph *g);
int64_t lf_dist_graph_num_launch_units(const lf_dist_graph *g);
/* cells whose upstream positions are not consecutive in the sweep order (they read through the index list) */
int64_t lf_dist_graph_num_noncontiguous(const lf_dist_graph *g);
int lf_dist_graph_get_layout(const lf_dist_graph *g, int32_t *perm, int32_t *phase_of_position);
int lf_dist_graph_get_csr(const lf_dist_graph *g, int32_t *ups_ptr, int32_t *ups_idx, int64_t *n_edges);
int lf_dist_graph_phase_range(const lf_dist_graph *g, int phase, int64_t out[2]);
int lf_dist_graph_round_counts(const lf_dist_graph *g, int round, int64_t out[4]); /* send t,b; recv t,b */
int lf_dist_graph_round_send_positions(const lf_dist_graph *g, int round, int side, int32_t *positions);
int64_t lf_dist_graph_round_recv_slot(const lf_dist_graph *g, int round, int side);

int lf_comm_unique_id(char id[128]);                 /* rank 0; broadcast the 128 bytes to the other ranks */
int lf_comm_create(const char id[128], int nranks, int rank, int device, lf_comm **out);
void lf_comm_destroy(lf_comm *c);
/* the same, returning what the communicator's teardown reports (an asynchronous error of an earlier Send / Recv) */
int lf_comm_close(lf_comm *c);

/* alpha / dx / alpha_floodplains: per LOCAL pixel (row-major over the rank's own rows) */
int lf_dist_router_create(const lf_dist_graph *g, const double *alpha, double beta, const double *dx,
                          double dx_scalar, double dt, const double *alpha_floodplains, int device,
                          lf_dist_router **out);
void lf_dist_router_destroy(lf_dist_router *r);
int64_t lf_dist_router_state_size(const lf_dist_router *r);
int64_t lf_dist_router_last_launches(const lf_dist_router *r);
/* schedule of the last fused phase that had cells on this router, as lf_router_last_fused_form: 1 time-major, 2 level
 * blocks, 3 levels (0: none yet) */
int lf_dist_router_last_fused_form(const lf_dist_router *r);
int lf_dist_router_to_engine_order(lf_dist_router *r, const double *src_pix_dev, double *dst_ord_dev);
int lf_dist_router_from_engine_order(lf_dist_router *r, const double *src_ord_dev, double *dst_pix_dev);
/* one kinematicWaveRouting call; q_ord_dev has lf_dist_router_state_size entries (local cells in engine
 * order followed by the ghost slots), lat_ord_dev the N local cells in engine order.  rank_top /
 * rank_bottom = -1 at the raster's edge.  Asynchronous on the library stream. */
int lf_dist_router_route(lf_dist_router *r, lf_comm *comm, double *q_ord_dev, const double *lat_ord_dev, int section,
                         int rank_top, int rank_bottom);
/* ncalls calls in a row (lat_ord_dev[s]: lateral inflow of call s), software-pipelined across calls: successive calls
 * alternate between the caller's state vector and a second one of the router, so phase 0 of call s + 1 runs beside the
 * later halo rounds of call s (second stream).  Same result as ncalls calls of lf_dist_router_route, in q_ord_dev.
 * lf_dist_router_compute_part_io is its building block: one part of a phase with the old discharge read from q_in and
 * everything else (new discharge, upstream values, ghost slots) in q_out. */
int lf_dist_router_route_many(lf_dist_router *r, lf_comm *comm, double *q_ord_dev, const double *const *lat_ord_dev, int ncalls,
                              int section, int rank_top, int rank_bottom);
int lf_dist_router_compute_part_io(lf_dist_router *r, const double *q_in_dev, double *q_out_dev, const double *lat_ord_dev,
                                   int section, int phase, int part);
/* One routing.dynamic() sub-step on the partition (= lf_routing_substep on the whole raster): element-wise stages on
 * the rank's own N cells, each router call with its halo exchanges.  engine_order = 1 (the rank's engine order);
 * a->ChanQKin and a->Chan2QKin are state vectors (lf_dist_router_state_size entries), all others have N entries. */
int lf_dist_routing_substep(lf_dist_router *r, lf_comm *comm, const lf_substep_args *a, int rank_top, int rank_bottom);
/* nsteps x routing.dynamic() on the partition (= lf_routing_substeps_fused on the whole raster, bit for bit): a rank
 * sweeps ONE PHASE for ALL sub-steps as a skewed wavefront over (level, sub-step); the router outputs that cross a
 * phase or a rank boundary are kept per sub-step in slabs [slot][sub-step], so there is ONE halo exchange per phase and
 * model step (RCCL Send/Recv of one contiguous block per neighbour and section) instead of one per phase, router call
 * and sub-step.  Vectors as lf_dist_routing_substep; sideflow_stride = 0 or N (one SideflowChanM3 vector per sub-step). */
int lf_dist_routing_substeps_fused(lf_dist_router *r, lf_comm *comm, const lf_substep_args *a, int nsteps,
                                   int64_t sideflow_stride, int rank_top, int rank_bottom);
/* its pieces (other transports, in-process loopback): allocate for nsteps; one phase; where a round's halo sits in the
 * slab of a section -- out = {send offset, send count, recv offset, recv count} in doubles; the RCCL exchange */
int lf_dist_fused_prepare(lf_dist_router *r, const lf_substep_args *a, int nsteps);
/* Several MODEL steps per call on the partition (= lf_routing_model_steps_fused on the whole raster, bit for bit): every phase
 * runs the sub-steps of all n_model_steps model steps as one wavefront and hands over the slabs of all of them in ONE halo
 * block, so the pipeline fill of a phase and the exchange round are paid once per call instead of once per model step.
 * a->SideflowChanM3: one vector per model step, sideflow_model_stride elements apart (0: one for all); a->sumDisDay:
 * [n_model_steps][N], zeroed by the caller.  _phase_model_steps: one phase of it (after lf_dist_fused_prepare for
 * steps_per_model_step * n_model_steps sub-steps), for callers that move the halo themselves. */
int lf_dist_routing_model_steps_fused(lf_dist_router *r, lf_comm *comm, const lf_substep_args *a, int steps_per_model_step,
                                      int n_model_steps, int64_t sideflow_model_stride, int rank_top, int rank_bottom);
int lf_dist_fused_phase_model_steps(lf_dist_router *r, const lf_substep_args *a, int steps_per_model_step, int n_model_steps,
                                    int64_t sideflow_model_stride, int phase);
int lf_dist_fused_phase(lf_dist_router *r, const lf_substep_args *a, int nsteps, int64_t sideflow_stride, int phase);
int lf_dist_fused_halo_block(const lf_dist_router *r, int round, int side, int64_t out[4]);
int lf_dist_fused_slab(const lf_dist_router *r, int section, void **slab_dev);
int lf_dist_fused_exchange(lf_dist_router *r, lf_comm *comm, int round, int split, int rank_top, int rank_bottom);
/* slab slots of the fused path: out[0] = slots, [1..2] first export slot top / bottom, [3..4] first ghost slot top /
 * bottom, [5] first slot of the local cells that feed a later phase; and the tables by position (tests) */
int lf_dist_graph_slab_layout(const lf_dist_graph *g, int64_t out[6]);
int lf_dist_graph_get_fused_tables(const lf_dist_graph *g, int32_t *out_slot, int32_t *ups_idx_f);
/* ups_base[N] by position, as the routers upload it: >= 0 = the cell's upstream cells are the consecutive run that starts
 * there, all of them ghost slots or local cells of the cell's own phase; -1 = they come from its list */
int lf_dist_graph_get_ups_base(const lf_dist_graph *g, int32_t *ups_base);
/* level blocks of the fused path (per phase, cone by cone): out = {blocks, blocks of more than one level, cones, entries
 * of the cone table}; all 0 when no block holds more than one level (then: one launch per level and sub-step wave) */
int lf_dist_graph_block_stats(const lf_dist_graph *g, int64_t out[4]);
/* the block plan of single router calls on the partition (one plan per stage = phase x {boundary-critical part, bulk};
 * blocks of launch units, each cut into cones of at most 64 cells per unit; see lf_blocks.h for the table layout):
 * sizes = {stages + 1, blocks + 1, rows, entries of the cone table, launch units + 1}; arrays may be NULL (sizes only) */
int lf_dist_graph_get_route_plan(const lf_dist_graph *g, int64_t sizes[5], int32_t *stage_block, int32_t *level,
                                 int32_t *row, int32_t *off, int32_t *cone, int64_t *level_start);
/* the same for the block plan of the fused sub-step path (one plan per phase): sizes = {phases + 1, blocks + 1, rows,
 * entries of the cone table} */
int lf_dist_graph_get_fused_plan(const lf_dist_graph *g, int64_t sizes[4], int32_t *phase_block, int32_t *level,
                                 int32_t *row, int32_t *off, int32_t *cone);
/* the pieces of a call, for transports other than RCCL and for tests */
int lf_dist_router_compute_phase(lf_dist_router *r, double *q_ord_dev, const double *lat_ord_dev, int section,
                                 int phase);
/* one part of a phase: 0 = its boundary-critical cells (the exports of the phase and what drains into them inside the
 * phase), 1 = the rest; the parts are independent, so lf_dist_router_route runs round j's halo exchange on a second
 * stream beside part 1 of phase j (LF_DIST_OVERLAP=0: one stream).  part_range: positions [begin, end) of a part. */
int lf_dist_router_compute_part(lf_dist_router *r, double *q_ord_dev, const double *lat_ord_dev, int section, int phase,
                                int part);
int lf_dist_graph_part_range(const lf_dist_graph *g, int phase, int part, int64_t out[2]);
int lf_dist_router_pack(lf_dist_router *r, const double *q_ord_dev, int round, void *send_ptr[2], int64_t send_count[2]);
int lf_dist_router_recv_slots(const lf_dist_router *r, int round, int64_t slot[2], int64_t count[2]);
int lf_dist_router_exchange(lf_dist_router *r, lf_comm *comm, double *q_ord_dev, int round, int rank_top,
                            int rank_bottom);

#ifdef __cplusplus
}
#endif
#endif /* LISFLOOD_AMD_H */
