/*
 * bader_hip.h -- C ABI of libbader_hip.so, the MI355X (gfx950) replacement for the hot path of
 * pybader v0.3.12: neargrid / ongrid steepest-ascent voxel->maximum assignment and the
 * edge-refinement sweep (pybader/methods.py, refinement.py, thread_handlers.py, the njit half of
 * utils.py).  Plain C types only; every function returns 0 on success or a negative XB_E_* code
 * with a message available from xb_last_error().  No C++ exception crosses this boundary.
 *
 * Data layout (the reference's, io/vasp.py:102-103): every grid array is C-order [x][y][z],
 * z fastest.  Density is float64; working labels ("volumes") are int32 on the device; `known`
 * edge flags are int8.  Host buffers are caller-owned numpy arrays; device buffers belong to the
 * context.  Label sentinels: -1 vacuum (utils.py:396-397), >=0 basin number after assignment.
 *
 * Each entry point cites the reference interface it replaces (file:line into pybader/).
 */
#ifndef BADER_HIP_H
#define BADER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xb_ctx xb_ctx;

enum { XB_OK = 0, XB_E_ARG = -1, XB_E_HIP = -2, XB_E_STATE = -3, XB_E_LIMIT = -4, XB_E_COMM = -5,
       XB_E_SHORT = -6 /* xb_parse_density_text / xb_parse_cube_text: fewer numbers in the text than the grid needs */ };

/* label dtype codes accepted at the boundary: the reference narrows/widens labels between
 * int8/16/32/64 (utils.py:15-37 dtype_calc, jits.py:22-38 dtype matrix) */
enum { XB_I8 = 1, XB_I16 = 2, XB_I32 = 4, XB_I64 = 8 };

/* methods.__contains__ (methods.py:12) */
enum { XB_METHOD_ONGRID = 0, XB_METHOD_NEARGRID = 1 };
/* refine_mode[0] (thread_handlers.py:144, 201-205) */
enum { XB_REFINE_ALL = 0, XB_REFINE_CHANGED = 1 };

/* ---- library / context ------------------------------------------------------------------ */
const char *xb_last_error(void);
int xb_device_count(void);                       /* number of visible HIP devices (0 = none) */
int xb_create(int device, xb_ctx **out);         /* one context per GPU; owns a stream + buffers */
void xb_destroy(xb_ctx *c);
int xb_sync(xb_ctx *c);                          /* hipStreamSynchronize on the context's stream */
void *xb_stream(xb_ctx *c);                      /* the hipStream_t every kernel is launched on */

/* ---- grid residency ---------------------------------------------------------------------- */
/* Declares the grid and the two small matrices the reference computes on the host with numpy and
 * passes to every kernel (Bader.distance_matrix interface.py:242-259, Bader.T_grad 285-290):
 * dist_mat[27] row-major [3][3][3] with index 2 == -1; T_grad[9] row-major.  Allocates/reuses
 * device buffers.  x-slab [x0,x1) is the range of axis-0 planes this context owns (multi-GPU
 * slab scheduler; x0=0,x1=nx for one GPU).  Every rank holds the full density.
 * SIZE LIMIT (the reference indexes with int64 throughout, methods.py / refinement.py): voxel indices are int32 on the
 * device, so a grid needs nx*ny*nz < 2^31 - 1 voxels (1024^3 = 2^30 fits; 1290^3 is the largest cube) -- more returns
 * XB_E_LIMIT before anything is allocated.  Every entry point works up to that size.
 * AXIS LIMITS: the tile launches put the tile counts of y and x into gridDim.y and gridDim.z, which the device bounds
 * (hipDeviceProp_t::maxGridSize, read when the context is created).  nx may be at most 4 * maxGridSize[2] (the 4-plane tiles of the
 * edge sweep and the relabel), ny at most 8 * maxGridSize[1] (the 8-row tiles of pass A, the edge sweep and the bricks): with
 * 65 536 for both, 262 144 and 524 288 voxels.  nz has no limit of its own.  A longer axis returns XB_E_LIMIT before anything is
 * allocated, with the axis and the limit in the message ("axis x of ... voxels exceeds the launch limit of ... voxels on x");
 * xb_axis_limits reads both limits.
 * An axis of one or two voxels (it meets itself through the wrap) is accepted for the transfers, xb_vacuum_assign and the weight
 * method; the assignment, refinement, table and sum entry points answer XB_E_ARG on such a grid. */
int xb_set_grid(xb_ctx *c, const int64_t shape[3], const double dist_mat[27], const double T_grad[9],
                int64_t x0, int64_t x1);
/* the longest x and y axis xb_set_grid accepts on this context's device (AXIS LIMITS above); host only */
int xb_axis_limits(xb_ctx *c, int64_t *nx_max, int64_t *ny_max);
int xb_upload_density(xb_ctx *c, const double *rho_host);           /* H2D, nx*ny*nz float64 */
/* workload generator, bit-identical to pybader_amd/synth.py (bench + tests; not in the reference) */
int xb_synth_density(xb_ctx *c, const double lattice[9], const double *atoms5, int64_t n_atoms,
                     double background);
int xb_download_density(xb_ctx *c, double *rho_host);
/* The density block of a VASP CHGCAR / CHG file (io/vasp.py:90-104, 147-149): `text` holds nx*ny*nz (or more)
 * whitespace separated decimal numbers in Fortran order (x fastest); they are converted exactly as numpy's
 * string -> float64 does (correctly rounded), divided by `divisor` (the cell volume) and stored as the
 * resident density rho[x][y][z].  The text is uploaded as it is and parsed on the device; tokens outside the
 * exact fast path are converted on the host (n_host of them, however many: a file written with 17 digits leaves
 * every one), in the C locale whatever LC_NUMERIC is.  Tokens after the grid's last number are ignored.
 * SURVEY.md 8(f) rank 4.
 * What converts: the tokens numpy's string -> float64 takes -- decimals with or without point and e / E exponent,
 * inf, infinity, nan in any letter case, each with an optional sign (a nan's sign and payload are not pinned) --
 * with two deliberate divergences: '_' between digits ("1_0") and non-ASCII digits, which numpy takes, are
 * refused; no writer emits them.  What numpy refuses is refused: hex floats, nan(...), a Fortran D exponent, ...
 * Errors of the two parse calls: XB_E_STATE no grid; XB_E_ARG an empty text, a bad divisor, nval or pick, an axis
 * below 3 voxels, a token among those used that does not convert; XB_E_SHORT fewer numbers than the grid needs;
 * XB_E_LIMIT a text of 2^43 bytes or more than 2^31 - 1 numbers; XB_E_HIP the runtime (out of memory, ...).
 * The resident density after a refused call: unchanged after every refusal but two -- after XB_E_ARG for a token
 * that does not convert, and after XB_E_HIP, it is unspecified (the values the device converted are already stored,
 * or added with `accumulate`; the host's are not): parse again in store mode, or upload, before using it. */
int xb_parse_density_text(xb_ctx *c, const char *text, int64_t nbytes, double divisor, int64_t *n_tokens,
                          int64_t *n_host);
/* The density block of a cube file (io/cube.py:93-123): `text` holds nx*ny*nz*nval (or more) whitespace separated
 * decimal numbers in C order, nval values per voxel (token i is voxel i / nval, value i % nval; line breaks do not
 * matter).  Only the tokens with i % nval == pick are converted (as xb_parse_density_text converts) and stored at
 * voxel i / nval of the resident density: x * scale, or (rho + x) * scale with `accumulate` -- a sum of values is a
 * chain of calls with scale 1 and the real scale on the last one, ((a + b) + c) * s left to right in float64.
 * XB_E_SHORT: fewer than nx*ny*nz*nval numbers; XB_E_LIMIT: nx*ny*nz*nval above 2^31 - 1; XB_E_ARG: a malformed
 * number among those converted, pick outside [0, nval). */
int xb_parse_cube_text(xb_ctx *c, const char *text, int64_t nbytes, int64_t nval, int64_t pick, int accumulate,
                       double scale, int64_t *n_tokens, int64_t *n_host);
/* ---- density -> text (CHGCAR / cube writers) ------------------------------------------------------------------------
 * io/vasp.py:167-250 (vasp.write) and io/cube.py:186-240 (cube.write) format the density with utils.python_format
 * (' {:.11E}' per value, utils.py:85-94) or utils.fortran_format (utils.py:40-82), one value at a time in Python.  Here the
 * values are formatted on the device, byte for byte as those functions do (csrc/fmt_core.h), and handed out as chunks of
 * whole lines.  The caller's array gets a device buffer of its own: the resident density and labels are left alone.
 *   xb_format_begin          values[x][y][z] float64 times `scale` (one IEEE multiply: `density *= lattice_vol`,
 *                            `charge *= bohr_to_ang**3`), in the file order of `layout`; style XB_STYLE_*, `prec` digits
 *                            after the point (11 CHGCAR, 5 cube); pow10[k - pow10_lo] = np.power(10.0, k) (the Fortran
 *                            style divides by numpy's powers).  n_host: values the device leaves to the host (nan, inf,
 *                            subnormals, magnitudes outside its exact range, uncertain floor(log10) in the Fortran style).
 *   xb_format_host_values    those values (already scaled) and their file-order indices, ascending
 *   xb_format_set_host_text  their text as the reference writes it: value i is text[offsets[i] .. offsets[i+1])
 *   xb_format_next           the next chunk (a pointer into a pinned buffer of the context, valid until the following
 *                            call); nbytes == 0 at the end.  The next chunk is formatted while the caller writes this one.
 *   xb_format_times          device time of the formatting kernels and of the chunk copies so far (ms)
 *   xb_format_end            frees the writer's buffers (also done by the next xb_format_begin and by xb_destroy) */
enum { XB_STYLE_E = 0 /* python_format */, XB_STYLE_E_SPACE = 1 /* python_format(a, p, ' ') */,
       XB_STYLE_F = 2 /* fortran_format */ };
enum { XB_TEXT_CHGCAR = 0 /* Fortran order (x fastest), 5 per line, a partial last line */,
       XB_TEXT_CUBE = 1 /* C order, every (x, y) record of nz values in lines of 6, a partial last line each */ };
int xb_format_begin(xb_ctx *c, const double *values, const int64_t shape[3], int layout, double scale, int style, int prec,
                    const double *pow10, int64_t pow10_lo, int64_t pow10_n, int64_t *n_host);
int xb_format_host_values(xb_ctx *c, int64_t *idx, double *vals);
int xb_format_set_host_text(xb_ctx *c, const int64_t *offsets, const char *text);
int xb_format_next(xb_ctx *c, void **data, int64_t *nbytes);
int xb_format_times(xb_ctx *c, double *format_ms, double *copy_ms);
int xb_format_end(xb_ctx *c);
/* labels: host <-> device with widening/narrowing on the device (utils.dtype_change, utils.py:255-259) */
int xb_upload_labels(xb_ctx *c, const void *labels_host, int dtype);
int xb_download_labels(xb_ctx *c, void *labels_host, int dtype);
int xb_upload_known(xb_ctx *c, const int8_t *known_host);
int xb_download_known(xb_ctx *c, int8_t *known_host);

/* ---- arrays that already live on the device ---------------------------------------------------------------------------
 * No counterpart in the reference (its arrays share one address space): the in-memory boundary for a caller whose density was
 * produced on the GPU (a torch / CuPy tensor; pybader_amd/device.py reads __cuda_array_interface__).  The library keeps its own
 * float64 C-order copy of the density, so every kernel's layout assumption and the parity guarantee hold.
 *   xb_import_density   the device array at dev_ptr -- dtype XB_F32 / XB_F64, the grid's shape, `stride` in ELEMENTS (any int64: 0
 *                       a broadcast axis, negative a flipped axis, dev_ptr then being the element [0][0][0]) -- becomes the
 *                       resident density: np.ascontiguousarray(a).astype(np.float64), a move plus an exact widening (every
 *                       finite value, +-inf and -0.0 bit for bit; a NaN stays a NaN).  Cached state as xb_upload_density.
 *                       Contiguous float64 is one device-to-device copy, contiguous float32 a vectorised widening, a permuted
 *                       layout (stride 1 on x or y) goes tile by tile through LDS, anything else is gathered voxel by voxel.
 *   xb_import_labels    xb_upload_labels from a C-contiguous device array of XB_I8 / I16 / I32 / I64
 *   xb_export_labels    xb_download_labels into one
 *   xb_export_volume    utils.volume_mask (utils.py:461-476) into a C-contiguous device array: XB_F64 the bits of
 *                       xb_volume_mask, XB_F32 that value rounded once
 *   xb_device_alloc / xb_device_free   result arrays the library owns (the device side of xb_host_alloc / xb_host_free);
 *                       xb_device_free waits for the device, so work still queued on the buffer ends first
 *   xb_device_read      `bytes` of a device array to host memory (returns with the data there)
 * CHECKS, all on the host before anything is queued, every failure XB_E_ARG: the pointer is device memory of the context's
 * device, every element the shape and strides address lies inside the ONE allocation that holds the pointer, the dtype is one of
 * those listed, the grid is set, and the array does not overlap the resident buffer it is copied from / into.  A wrong stride is
 * an error code, never a memory fault; a refused call leaves the context as it was.
 * ORDER: `stream` is the caller's hipStream_t (null: the legacy default stream).  The work starts after everything queued on
 * `stream` so far and `stream` goes on after it (events in both directions): a source may be overwritten or freed, a destination
 * read, on `stream` right after the call returns.  None of these calls adds a wait of the host (xb_import_labels keeps the
 * one of xb_upload_labels, xb_device_read returns data). */
enum { XB_F32 = 32, XB_F64 = 64 };
int xb_import_density(xb_ctx *c, const void *dev_ptr, int dtype, const int64_t stride[3], void *stream);
int xb_import_labels(xb_ctx *c, const void *dev_ptr, int dtype, void *stream);
int xb_export_labels(xb_ctx *c, void *dev_ptr, int dtype, void *stream);
int xb_export_volume(xb_ctx *c, int64_t vol_num, void *dev_ptr, int dtype, void *stream);
int xb_device_alloc(int device, int64_t bytes, void **out);
int xb_device_free(void *p);
int xb_device_read(xb_ctx *c, void *dst_host, const void *dev_ptr, int64_t bytes, void *stream);

/* ---- hot path, device resident ----------------------------------------------------------- */
/* utils.vacuum_assign (utils.py:382-401) via Bader.volumes_init (interface.py:449-469):
 * labels := 0, then -1 where rho <= vac_tol (vac_tol NaN => no vacuum, the vacuum_tol=None case).
 * Returns the vacuum charge (sum(rho)*voxel_volume) and volume. */
int xb_vacuum_assign(xb_ctx *c, double vac_tol, double voxel_volume, double *vac_charge, double *vac_volume);

/* thread_handlers.bader_calc (thread_handlers.py:15-75) with methods.neargrid (methods.py:222-611)
 * or methods.ongrid (methods.py:15-219): labels (0 / -1 on entry) become 0-based basin numbers,
 * numbered by the smallest C-order voxel index of each basin (the order the reference's scan
 * discovers maxima).  neargrid computes every voxel's own dr=0 trajectory -- the order-independent
 * map the reference's refinement converges to.
 * n_maxima: number of basins.  With several slabs the numbering is completed by
 * xb_assign_finish after the per-rank maxima tables were merged.
 * XB_E_LIMIT: more maxima than the maxima table holds, min(N, 2^22) = 4 194 304 entries ("<count> maxima exceed the table
 * capacity <capacity>"; exactly 2^22 maxima still fit).  The labels and xb_get_maxima's list are undefined after this refusal;
 * nothing else is lost: the density stays resident, and the caller may upload another density or assign again (either method)
 * on the same context -- it returns what a fresh context returns and holds the device memory a fresh one holds (xb_memory_stats). */
int xb_assign(xb_ctx *c, int method, int64_t *n_maxima);
/* bader_max of thread_handlers.py:75: voxel indices int64[n][3] in label order */
int xb_get_maxima(xb_ctx *c, int64_t *maxima_out, int64_t capacity);

/* slab scheduler pieces of xb_assign (multi-GPU): phase 1 traces the owned slab and returns the
 * local table (maximum voxel index, smallest owned voxel index reaching it); the host merges the
 * tables of all ranks (min over ranks), sorts, and hands the global table back to phase 2. */
int xb_assign_trace(xb_ctx *c, int method, int64_t *n_local);
int xb_assign_local_table(xb_ctx *c, int64_t *max_idx, int64_t *first_idx, int64_t capacity);
int xb_assign_finish(xb_ctx *c, const int64_t *max_idx_sorted, int64_t n_global);

/* optional, before the first xb_edge_find of a refinement: build what xb_refine_trace needs (the gradient-field
 * table of the resident density) now, so that edge_find can read "not a maximum" off it (xb_refine does it) */
int xb_prepare_refine(xb_ctx *c);
/* refinement.edge_find (refinement.py:326-405) on a fresh `known`: -2 edge, -1 within the 27-box
 * of an edge, 2 other non-vacuum, 0 untouched vacuum.  Returns the edge count of the owned slab. */
int xb_edge_find(xb_ctx *c, int64_t *edges);
/* refinement.neargrid (refinement.py:17-322): retrace every known==-2 voxel of the owned slab
 * until a known==2 voxel or a maximum; relabel the start voxel if the label differs.
 * escaped: traces that left the valid x-range [x0-halo, x1+halo) (slabs only; 0 on one GPU). */
int xb_refine_trace(xb_ctx *c, int64_t *changed, int64_t *escaped);
/* slab fallback: escaped traces are parked as known == -6; after the scheduler made the whole grid
 * valid on this rank (all-gather of labels + known, xb_set_halo(nx)) this call retraces exactly them. */
int xb_refine_trace_escaped(xb_ctx *c, int64_t *changed, int64_t *escaped);
/* slab scheduler, escaped retraces without bulk traffic: the dr=0 trajectory of every parked voxel
 * (known == -6) of the owned slab -- it depends on the replicated rho only -- from the point where it first
 * leaves this rank's valid planes (the fast retrace already walked the part before without finding a stop).
 * The scheduler asks the owners of the path voxels for (label, known) with xb_gather_voxels, finds the first
 * known == 2 voxel (refinement.py:294-303) or the maximum, and writes the outcome back with
 * xb_scatter_voxels.  Layout: offsets has n_paths + 1 entries; voxels[offsets[i]] is the start voxel of path
 * i, the rest of path i follows (linear indices).  Trajectories are followed for at most max_len voxels;
 * complete[i] = 1 when path i reached its maximum, else ask again with a larger max_len. */
int xb_escaped_paths(xb_ctx *c, int64_t max_len, int64_t *n_paths, int64_t *n_voxels);
int xb_escaped_paths_fetch(xb_ctx *c, int64_t *starts, int64_t *offsets, int64_t *voxels, int8_t *complete);
int xb_gather_voxels(xb_ctx *c, const int64_t *idx, int64_t n, int32_t *labels_out, int8_t *known_out);
/* xb_scatter_voxels may write any voxel, so it invalidates what the context has cached of the labels: the edge and changed-voxel
 * lists, the per-brick label marks of the last assignment (uniformity, the trapping regions' labels) and xb_vacuum_assign's
 * promise that the -1 labels are exactly the voxels at or below its tolerance (the next assignment walks every brick again).  A
 * negative label among the written ones makes the next assignment treat the grid as one with vacuum (-1 labels stay).  The
 * halo's wire width grows only if a written label does not fit it (xb_label_wire).  The table and the density's results stay. */
int xb_scatter_voxels(xb_ctx *c, const int64_t *idx, int64_t n, const int32_t *labels_in, const int8_t *known_in);
/* slab scheduler, escaped retraces carried on by their next owner.  A retrace that leaves this rank's valid planes is
 * parked (known == -6) and exported as a walker: XB_WALKER_WORDS int64 holding its start voxel and label, the voxel it
 * arrived at, the carried remainder, the path window and the step count (refinement.py:137-154, 200-235: everything
 * the loop carries).  The scheduler all-gathers the walkers; xb_walkers_continue carries on the ones that arrived on a
 * plane this rank owns (its labels / known are the authoritative ones there: a retrace only reads labels at known == 2
 * voxels and maxima, which no retrace rewrites) and yields results -- int64 pairs (start voxel | final label << 32) --
 * and the walkers that left its valid planes again; xb_walkers_apply applies the pairs whose voxel this rank owns
 * exactly as the retrace would have (refinement.py:288-291).  A walker that needs the exact slow path (path window
 * overflow) comes back as `stuck` and stays parked for xb_escaped_paths.  The reference has no counterpart: its
 * thread blocks read one shared array (thread_handlers.py:128-236). */
#define XB_WALKER_WORDS 10
int xb_walkers_count(xb_ctx *c, int64_t *n_walkers, int64_t *n_results);
int xb_walkers_fetch(xb_ctx *c, int64_t *walkers, int64_t *results);
int xb_walkers_continue(xb_ctx *c, const int64_t *walkers, int64_t n);
int xb_walkers_apply(xb_ctx *c, const int64_t *results, int64_t n, int64_t *changed, int64_t *stuck);
/* refinement.edge_check (refinement.py:409-508), bug-compatible (no vacuum test on the box voxels).
 * No size limit of its own below xb_set_grid's (round 6: the two flag bits of a queue entry moved out of the voxel's 32-bit
 * word; rounds 1-5 stopped at 2^30 voxels, exactly 1024^3). */
int xb_edge_check(xb_ctx *c, int64_t *checked, int64_t *edges);
/* refinement.edge_check across slabs ('changed' refinement on N GPUs): the greedy scan of refinement.py:420-427 is
 * global, so every rank resolves the global list of changed voxels.  _local: the owned changed voxels and their
 * edge&maximum class; _local_fetch copies them out; _global takes the all-gathered lists (label and known halos
 * refreshed before), resolves them and re-classifies the boxes that touch this rank's planes; `edges` counts the new
 * edges in the owned planes (the scheduler sums over ranks). */
int xb_edge_check_local(xb_ctx *c, int64_t *n_out);
int xb_edge_check_local_fetch(xb_ctx *c, int64_t *idx_out, int8_t *cls_out);
int xb_edge_check_global(xb_ctx *c, const int64_t *idx, const int8_t *cls, int64_t n, int64_t *checked, int64_t *edges);
/* thread_handlers.refine (thread_handlers.py:128-236): the iteration driver on one GPU.
 * iters < 0 => until nothing changes.  log[2*k] = edges, log[2*k+1] = changed of iteration k+1. */
int xb_refine(xb_ctx *c, int mode, int64_t iters, int64_t *log, int64_t log_capacity, int64_t *n_iters);
/* Bader.bader_calc + Bader.refine_volumes back to back, as Bader.__call__ issues them (interface.py:406-416, 471-490), in ONE call:
 * the refinement's first iteration is queued behind the assignment and one host wait serves both.  Results, maxima (xb_get_maxima)
 * and log equal xb_assign followed by xb_refine; combinations other than the one-GPU neargrid path without vacuum, and assignments
 * that do not end the usual way (tie voxels, walkers for the exact slow path, more than 2048 maxima), run as those two calls.
 * XB_E_LIMIT: more than min(N, 2^22) maxima, as xb_assign states it, with the same leave to upload or assign again afterwards. */
int xb_assign_refine(xb_ctx *c, int method, int mode, int64_t iters, int64_t *n_maxima, int64_t *log, int64_t log_capacity, int64_t *n_iters);

/* utils.charge_sum (utils.py:235-252) via Bader.sum_volumes (interface.py:492-525) */
int xb_charge_sum(xb_ctx *c, double voxel_volume, int64_t n_labels, double *charge, double *volume);
/* ---- moments of the density per label about a centre (atomic dipoles and quadrupoles; the multipole module of the Henkelman
 * group's `bader` program) -- no counterpart in the reference ----
 * Next to xb_charge_sum: one pass over the owned planes [x0, x1) of the resident density and labels (a slab rank gets its partial
 * sums); nothing resident is written.  lattice[9]: the cell, a row per axis; centres_cart[n][3]: the centre of label a, Cartesian.
 * Every owned voxel v = (p0, p1, p2) whose label a satisfies 0 <= a < n contributes (labels < 0 and >= n are skipped):
 *   position  as utils.surface_dist (utils.py:357-359), left to right:
 *             pc[j] = lat[j]*p0/nx;  pc[j] += lat[3+j]*p1/ny;  pc[j] += lat[6+j]*p2/nz
 *   image     the 27 images x, y, z = -1..1 in that nesting order, pbc[j] = (lat[j]*x + lat[3+j]*y) + lat[6+j]*z,
 *             e[j] = pc[j] - (centre[a][j] + pbc[j]),  d2 = (e0*e0 + e1*e1) + e2*e2;  the image kept is the first with a strictly
 *             smaller d2, starting from the largest double (a tie keeps the earlier image);  d[j] = the e[j] of that image
 *   terms     with w = rho[v] and t_j = w*d[j] formed first:
 *             w,  t_0, t_1, t_2,  t_0*d0, t_0*d1, t_0*d2,  t_1*d1, t_1*d2,  t_2*d2
 *   result    moments[a][0..9] = the ten sums of these terms over the label's voxels, each multiplied once by voxel_volume
 *             (m0; m1 x y z; m2 xx xy xz yy yz zz);  volume[a] = the voxel count times voxel_volume
 * The terms are a pure function of their inputs (no contraction); the order of the sums is free (float atomics, as xb_charge_sum).
 * n <= 224 labels sum in LDS bins per block, more in global memory; waves that hold one label add once per wave.
 * XB_E_STATE: no grid, or a grid that has received no density or no labels yet;  XB_E_ARG: n < 1 or a null pointer;
 * XB_E_LIMIT: n above (2^31 - 1) / 10.  XB_TIMER_MOMENTS of xb_kernel_time; its buffer is counted by xb_memory_stats. */
int xb_moment_sum(xb_ctx *c, const double lattice[9], const double *centres_cart, int64_t n, double voxel_volume,
                  double *moments /* n*10 */, double *volume /* n */);
/* ---- which labels share a surface: facet counts and the saddle per pair of labels (interatomic surfaces, the grid estimate of the
 * bond critical point, the barrier a persistence filter of spurious maxima needs) -- no counterpart in the reference ----
 * Next to xb_charge_sum: two passes over the resident density rho (the field the labels were made from) and the resident labels of
 * the whole grid; nothing resident is written.  n: the number of labels; dirs[n_dirs][3]: the active directions, each in
 * {-1,0,1}^3 \ {0}, none twice or with its negative (pybader_amd.adjacency.active_directions: of the 13 offsets d > -d in tuple
 * order those whose facet of the voxel lattice's Voronoi cell has an area >= 1e-10 * V_voxel^(2/3), ascending: 3 for an orthogonal
 * cell, up to 7 for a triclinic one).
 *   facets    every voxel v = (p0, p1, p2) owns, for each direction k, the facet towards u = v + d_k, wrapped periodically on every
 *             axis; its id is f = lin(v) * 8 + k with lin the C-order index (unique for n_dirs <= 8).  The facet counts when
 *             a = label[v] and b = label[u] both lie in [0, n) and a != b; its pair is (min(a, b), max(a, b)).  Labels < 0 and >= n
 *             make a facet count for nothing.  An axis of length 1 gives no facets along it (u == v); an axis of length 2 gives two
 *             facets between the same two voxels, one owned by each, and both count.
 *   per pair  facets[k]: the number of its facets in direction k;  saddle: the maximum over its facets of s = the smaller of
 *             rho[v], rho[u], "smaller" and "maximum" both in the total order of key(x) = bits(x) ^ (bits(x) >> 63 ? ~0 : 1 << 63)
 *             compared as uint64 (it equals < on ordinary values, puts -0.0 below +0.0 and is defined for NaN);  saddle_facet: the
 *             smallest facet id among the pair's facets whose s has the maximal key
 *   result    the pairs in ascending (a, b).  Counts are integers, the saddle a maximum of existing bits, ties go to an index:
 *             nothing depends on scheduling and every number is exact.
 * n <= 256 labels use a triangular table in global memory, more an open-addressing hash table (key a << 32 | b, 64-bit
 * compare-and-swap) that a counting pass sizes: a power of two >= twice the counting facets.  The table is allocated on demand, kept
 * while the grid's shape stays, counted by xb_memory_stats and freed by xb_adjacency_release.  The occupied entries are compacted on
 * the device and sorted by key on the host.
 *   xb_adjacency_fetch   the pairs of the last call: a[i] < b[i], facets[i * n_dirs + k], saddle[i], saddle_facet[i]
 * XB_E_STATE: no grid, a grid that has received no density or no labels yet, a context that holds a slab (fetch: no result);
 * XB_E_ARG: n < 1, n_dirs outside 1..13, a direction outside {-1,0,1}^3 \ {0}, given twice or together with its negative, a null
 * pointer, capacity < n_pairs in fetch;  XB_E_LIMIT: n > 2^31 - 1.  XB_TIMER_ADJACENCY of xb_kernel_time. */
int xb_adjacency(xb_ctx *c, const int32_t *dirs /* n_dirs*3 */, int n_dirs, int64_t n, int64_t *n_pairs);
int xb_adjacency_fetch(xb_ctx *c, int32_t *a, int32_t *b, int64_t *facets /* cap*n_dirs */, double *saddle,
                       int64_t *saddle_facet, int64_t capacity);
int xb_adjacency_release(xb_ctx *c);
/* ---- merge Bader volumes below a persistence threshold (the filter of spurious maxima the saddles above are for) -- no
 * counterpart in the reference ----
 * Reads the resident density rho (the field the labels were made from) and the resident labels of the whole grid; nothing
 * resident is written.  n: the number of labels; dirs[n_dirs][3]: exactly the active directions of xb_adjacency, under the same
 * checks; max_idx[n]: the linear C-order voxel of each label's maximum; tol; max_rounds.  Every quantity is exact.
 *   notation  key() is the total order of xb_adjacency;  peak[m] = rho[max_idx[m]];  label b is ABOVE a iff key(peak[b]) >
 *             key(peak[a]), or the keys are equal and b < a: a strict total order on the labels.  (pybader_amd.adjacency.persistence
 *             puts two maxima of the same bits above neither.  Here one is above the other on purpose: a plateau split into two
 *             maxima must be able to merge, and parents strictly above their children make the parent pointers a forest.)
 *   state     cur[m], the current root of the original label m; at first m
 *   a round   facets, wrapping, the rules for axes of length 1 and 2 and "labels < 0 or >= n count for nothing" are those of
 *             xb_adjacency.  The facet (v, k) with u = v + d_k has A = cur[label[v]], B = cur[label[u]] and counts when both lie in
 *             [0, n) and A != B; then sk = the smaller key of rho[v], rho[u], `lower` is the one of A, B the other is above and
 *             `upper` the other.  Per root m that was `lower` on a counting facet: best[m] = the largest sk, target[m] = the smallest
 *             label among the `upper`s of the facets with sk == best[m], pers[m] = peak[m] - unkey(best[m]) (one float64
 *             subtraction); every other root has pers[m] = +inf.  m merges iff pers[m] < tol (false for a NaN): parent[m] =
 *             target[m], else parent[m] = m.  cur'[m] = the end of the parent chain from cur[m].
 *   rounds    repeat until one merges nothing or max_rounds have run.  Integer atomics in any order give the same result.
 *   results   rounds, n_survivors, converged (the last round merged nothing); per original label m (xb_merge_fetch): root[m] = the
 *             final cur[m];  merge_round[m] = the round, from 0, in which the root m merged, -1 if it survives;
 *             merge_persistence[m] = pers[m] of that round, for a survivor of the last round run.  A label no voxel carries has no
 *             facet and survives as its own root.
 * Per round two streaming passes shaped as xb_adjacency's (atomic max of sk into best[lower]; atomic min of `upper` into
 * target[lower]) and a kernel per label; the roots are found by pointer doubling; one host wait per round.  The current root
 * reaches the passes by a gather through an n-entry table, read only by lanes on a boundary of the original labels.  Its buffer,
 * 44 bytes per label, is allocated on demand, kept while the grid's shape stays, counted by xb_memory_stats and freed by
 * xb_merge_release.
 * XB_E_STATE: no grid, a grid that has received no density or no labels yet, a context that holds a slab (fetch: no result);
 * XB_E_ARG: the direction faults of xb_adjacency, n < 1, a null pointer, max_rounds < 1, tol negative or NaN (+inf is allowed), a
 * max_idx outside [0, N), capacity < n in fetch;  XB_E_LIMIT: n > 2^31 - 1.  All found on the host before any launch.
 * XB_TIMER_MERGE of xb_kernel_time. */
int xb_merge_basins(xb_ctx *c, const int32_t *dirs, int n_dirs, int64_t n, const int64_t *max_idx, double tol, int64_t max_rounds, int64_t *rounds, int64_t *n_survivors, int *converged);
int xb_merge_fetch(xb_ctx *c, int32_t *root, int32_t *merge_round, double *merge_persistence, int64_t capacity);
int xb_merge_release(xb_ctx *c);
/* ---- the weight method (Yu & Trinkle, J. Chem. Phys. 134, 064111; `bader -b weight`) -- no counterpart in the reference ----
 * Charge and volume per maximum with the surface voxels split fractionally, next to xb_charge_sum.  The resident density is the
 * partition field rho, the resident labels are read for their -1 marks (vacuum: absent, sends and receives nothing); neither is
 * written.  alpha[27]: the neighbour weights facet area / distance of the voxel lattice's Voronoi cell (pybader_amd.weight.
 * voronoi_weights), row-major [3][3][3] with index 2 == -1 like dist_mat, centre 0, symmetric bit for bit, finite, >= 0.
 *   flux          f_ij = alpha_d * max(rho_j - rho_i, 0), S_i = sum_d f_ij in the table's C order, J_ij = f_ij / S_i;
 *                 S_i == 0: voxel i is a maximum (every voxel of a plateau is its own)
 *   accumulation  A_i = q_i + sum_d J_ji * A_j over the neighbours with f_ji > 0, same order; V_i with 1 for q_i
 *   result        per maximum m, in ascending voxel index: A_m * voxel_volume, V_m * voxel_volume
 * A pure function of its inputs (one writer per A_i, fixed order, no contraction): bit-identical to a float64 loop that visits
 * the voxels in ascending rho.  The integrand q: q_host (nx*ny*nz float64, C order), NULL for rho itself, or with
 * xb_weight_sum_device a device array under the CHECKS and ORDER of xb_import_density.
 * XB_E_STATE: no grid, a context that holds a slab, or voxels left over on an empty frontier (a NaN in the density).
 *   xb_weight_fetch   the results of the last call: linear voxel index, charge, volume of each maximum
 *   xb_weight_stats   out = {levels, levels run as batched launches, levels run in the single-workgroup tail, batches (host waits
 *                     of the level loop), voxels finished, largest frontier handed on by a batched level, device bytes of the
 *                     method's own buffers (also counted by xb_memory_stats)} */
int xb_weight_sum(xb_ctx *c, const double alpha[27], double voxel_volume, const double *q_host, int64_t *n_maxima);
int xb_weight_sum_device(xb_ctx *c, const double alpha[27], double voxel_volume, const void *dev_ptr, int dtype,
                         const int64_t stride[3], void *stream, int64_t *n_maxima);
int xb_weight_fetch(xb_ctx *c, int64_t *max_idx, double *charge, double *volume, int64_t capacity);
int xb_weight_stats(xb_ctx *c, int64_t out[7]);
/* frees the method's device buffers (25 N bytes, kept between calls while the grid stays) and the fetched results */
int xb_weight_release(xb_ctx *c);
/* ---- the Voronoi partition: every voxel to its nearest atom (`bader -c voronoi` in the Henkelman group's code; the geometric
 * baseline next to the Bader charges, and a second atom map for xb_charge_sum, xb_moment_sum, xb_adjacency, xb_volume_mask) -- no
 * counterpart in the reference ----
 * WRITES the resident labels of the whole grid, as xb_upload_labels does, and invalidates everything that call invalidates (edge
 * list, cached sums, the vacuum-by-tolerance mark, brick uniformity, the label width of the halos).  lattice[9]: the cell, a row per
 * axis; atoms_cart[n][3]: Cartesian, already minus the voxel offset.  All of it is IEEE float64 without contraction: bit-defined.
 *   position  of voxel (p0, p1, p2), as xb_moment_sum's and utils.surface_dist's (utils.py:357-359), left to right:
 *             pc[j] = lat[j]*p0/nx;  pc[j] += lat[3+j]*p1/ny;  pc[j] += lat[6+j]*p2/nz
 *   distance  for atom a and image x, y, z = -1..1, pbc[j] = (lat[j]*x + lat[3+j]*y) + lat[6+j]*z:
 *             e[j] = pc[j] - (atom[a][j] + pbc[j]),  d2 = (e0*e0 + e1*e1) + e2*e2
 *   label     D(a) = the minimum of d2 over the 27 images; the voxel's label is the a with the smallest D(a), TIES GO TO THE SMALLER
 *             ATOM INDEX: the lexicographic minimum of (d2, a) over all 27 n pairs, which no order of the search changes.  Only
 *             these 27 images of the positions as given are searched; atoms are not wrapped into the cell.
 *   vacuum    with vac_tol not NaN a voxel with rho <= vac_tol gets -1, as xb_vacuum_assign decides it; with NaN the density is
 *             not read at all (a context without one is accepted).
 * One workgroup per 8 x 8 x 8 tile of voxels.  It keeps the images whose distance from the tile's centre is at most d_min + 2 R +
 * slack (d_min the smallest such distance, R the tile's circumradius: no other image can be nearest, or tied for it, at any voxel of
 * the tile; csrc/k_cell.h derives the slack), compacts them into LDS and lets every voxel search those.  A tile that keeps more
 * than XB_VORONOI_CAND_MAX images searches all 27 n from global memory; XB_VORONOI_FULL_SEARCH in `flags` makes every tile do so:
 * the second implementation, for tests and benchmarks -- both give the same labels.
 *   stats     NULL, or {tiles answered from a candidate list, tiles answered by the full search, the largest number of images a
 *             tile kept (it may exceed the cap; 0 with XB_VORONOI_FULL_SEARCH)}.  The call ends with a wait for the device.
 * XB_E_STATE: no grid, a vacuum tolerance on a grid that has received no density yet, a context that holds a slab;
 * XB_E_ARG: n < 1, a null lattice or atoms pointer, unknown flag bits, a lattice entry or coordinate that is not finite;
 * XB_E_LIMIT: n > (2^31 - 1) / 27.  No timer slot: a caller times the call.  Its buffer is counted by xb_memory_stats. */
enum { XB_VORONOI_FULL_SEARCH = 1, XB_VORONOI_CAND_MAX = 512 };
int xb_voronoi_assign(xb_ctx *c, const double lattice[9], const double *atoms_cart, int64_t n, double vac_tol, int flags,
                      int64_t stats[3]);
/* ---- critical points of the density and the bond graph they define (the core of a QTAIM analysis: nuclear, bond, ring and cage
 * points; which atoms a bond path joins and rho at the bond point) -- no counterpart in the reference ----
 * Reads the resident density rho of the whole grid (xb_critical_bonds the resident labels too); nothing resident is written.  The
 * points are the PIECEWISE-LINEAR critical points of rho on the Freudenthal (Kuhn) triangulation of the periodic voxel lattice:
 * combinatorial, integer-exact, and on a grid with every axis >= 4 they satisfy minima - sum ring + sum bond - maxima == 0 (the
 * Euler characteristic of the 3-torus) for ANY field, noise and plateaus included.
 *   order     lin is the C-order index, key() the total order of xb_adjacency;  u < v ("u is below v") iff key(rho[u]) < key(rho[v]),
 *             or the keys are equal and lin(u) < lin(v)
 *   offsets   d_0 .. d_6 = (0,0,1) (0,1,0) (0,1,1) (1,0,0) (1,0,1) (1,1,0) (1,1,1),  d_{7+k} = -d_k;  u_k = v + d_k, wrapped on every axis
 *   masks     bit k of L(v) is set iff u_k is below v -- strictly: a neighbour that wraps onto v itself leaves its bit clear;
 *             U(v) = ~L(v) & 0x3fff
 *   link      bits a and b are adjacent iff d_b - d_a, as an integer vector without wrapping, is one of the 14 offsets: 36 edges and
 *             24 triangles, a triangulated sphere.  c(M) = the number of connected components of the set bits of M (at most 6)
 *   kind      L == 0: a minimum (cage point);  U == 0: a maximum (nuclear point);  otherwise ring = c(L) - 1 is the multiplicity of
 *             the voxel as a 1-saddle and bond = c(U) - 1 as a 2-saddle; regular when both are 0.  A voxel may be both (on noise)
 *   counts    counts[XB_CRITICAL_*] = {maxima, bond voxels, sum of bond, ring voxels, sum of ring, minima};  with every axis >= 4:
 *             minima - sum ring + sum bond - maxima == 0.  Below 4 the wrapped neighbours coincide; the definition stands as
 *             written, the identity is not claimed
 *   vacuum    with vac_tol not NaN a voxel with rho[v] <= vac_tol is neither counted nor listed; its density still enters its
 *             neighbours' masks.  The identity is not promised then
 *   list      one record per non-regular voxel, ascending in lin: (lin, L, ring, bond), ring = bond = 0 for the two extrema.  Never
 *             cut short: xb_critical_points returns its length, xb_critical_fetch wants that capacity
 *   table     xb_critical_lut: out[L] = ring | bond << 4 for every L, 0 for L == 0 and L == 0x3fff; host only, needs no GPU
 * The maxima use the 14-neighbour test: a superset of the 26-neighbour maxima of xb_assign.
 *   bonds     xb_critical_bonds(n) works on the list of the last xb_critical_points call of this context (any writer of the density
 *             discards it) and the resident labels.  For every listed voxel v with bond > 0 and every component of U(v): its TOP is
 *             the greatest neighbour of the component in the order above, its basin labels[top].  D(v) = the distinct basins in
 *             [0, n) (labels < 0 and >= n count for nothing).  Every unordered pair a < b of D(v) gains one saddle; per pair:
 *             saddles, the count;  rho_b, the maximum of rho[v] under key();  voxel, the smallest lin among its bond voxels with that
 *             key.  A bond voxel with exactly one basin in D(v) counts towards same_basin: its bond path returns to the basin it
 *             left, through a periodic image or inside a noisy basin.  Pairs ascending in (a, b).  Integers and maxima of existing
 *             bits only.
 * One streaming pass: a workgroup stages the keys of an 8 x 8 x 32 tile and its halo in LDS, 14 ordered comparisons per voxel, one
 * byte of the table (global memory); a wave of regular voxels leaves after one ballot.  XB_CRITICAL_FLOOD in `flags` counts the
 * components by a flood fill in registers instead: the second implementation, same results.  The records are compacted on the
 * device -- into a list of N / 64 + 4096 records that a call with more grows to the number its own counter found before it runs
 * again -- and sorted on the host; a second kernel over the listed bond voxels emits the tops' labels, the host reduces per pair.
 * XB_E_STATE: no grid, no density (bonds: no labels, no list) on this grid yet, a context that holds a slab (fetch: no result);
 * XB_E_ARG: a null pointer, unknown flag bits, n < 1, capacity below the length in a fetch.  No timer slot: a caller times the
 * calls.  The list and the table are counted by xb_memory_stats and freed by xb_critical_release. */
enum { XB_CRITICAL_FLOOD = 1 };
enum { XB_CRITICAL_MAXIMA = 0, XB_CRITICAL_BOND_VOXELS = 1, XB_CRITICAL_BOND_SUM = 2, XB_CRITICAL_RING_VOXELS = 3,
       XB_CRITICAL_RING_SUM = 4, XB_CRITICAL_MINIMA = 5, XB_CRITICAL_COUNTS = 6 };
enum { XB_CRITICAL_FULL = 16383 /* 0x3fff: every neighbour below */, XB_CRITICAL_LUT_SIZE = 16384 };
int xb_critical_lut(uint8_t out[16384]);
int xb_critical_points(xb_ctx *c, double vac_tol, int flags, int64_t counts[6], int64_t *n_list);
int xb_critical_fetch(xb_ctx *c, int64_t *lin, uint16_t *lower_mask, uint8_t *ring, uint8_t *bond, int64_t capacity);
int xb_critical_bonds(xb_ctx *c, int64_t n, int64_t *n_pairs, int64_t *same_basin);
int xb_critical_bonds_fetch(xb_ctx *c, int32_t *a, int32_t *b, int64_t *saddles, double *rho_b, int64_t *voxel, int64_t capacity);
int xb_critical_release(xb_ctx *c);
/* ---- the Laplacian and the Hessian of the density: as a field, summed per label, and at listed voxels (the sign of the Laplacian
 * and the ellipticity at a bond point; L(Omega), the integral of the Laplacian over a basin, which vanishes over an exact zero-flux
 * basin and is the figure of merit AIM codes print next to the charge) -- no counterpart in the reference ----
 * All three calls read the resident density rho of the whole grid (xb_laplacian_sum the resident labels too); nothing resident is
 * written.  lattice[9]: the cell, a row per axis.  The stencil is the compact second-order one on 19 points: the voxel, its six
 * axis neighbours and its twelve edge neighbours, every coordinate wrapped.
 *   geometry  A[i][j] = lattice[3*i+j] / n_i (the voxel lattice, one row per axis; n_0 n_1 n_2 = nx ny nz);  M = the inverse of A,
 *             so that dp_i / dr_alpha = M[alpha][i] for the voxel coordinate p and the Cartesian r;  G = M^T M.  In this order:
 *               C[i][a] = A[i+1][a+1]*A[i+2][a+2] - A[i+1][a+2]*A[i+2][a+1]        (the cofactors; indices mod 3)
 *               det     = (A[0][0]*C[0][0] + A[0][1]*C[0][1]) + A[0][2]*C[0][2]
 *               M[a][i] = C[i][a] / det
 *               G[i][j] = (M[0][i]*M[0][j] + M[1][i]*M[1][j]) + M[2][i]*M[2][j]
 *   voxel     rho(+i) is the periodic neighbour along axis i, rho(+i+j) the periodic edge neighbour, c = rho(p):
 *               d_ii = (rho(+i) - c) + (rho(-i) - c)
 *               d_ij = (rho(+i+j) - rho(+i-j)) - (rho(-i+j) - rho(-i-j))           for ij in 01, 02, 12 (the 1/4 is in the coefficient)
 *               g_i  = rho(+i) - rho(-i)                                           (the 1/2 is in the coefficient)
 *   values    every sum left-associated in the term order k = 00, 11, 22, 01, 02, 12:  ((((x_0 + x_1) + x_2) + x_3) + x_4) + x_5
 *               Laplacian           sum w_k d_k,        w_ii = G[i][i],  w_ij = 0.5 * G[i][j]
 *               Hessian ab          sum h_ab,k d_k,     h_ab,ii = M[a][i]*M[b][i],  h_ab,ij = 0.25 * (M[a][i]*M[b][j] + M[a][j]*M[b][i]),
 *                                   ab in xx, xy, xz, yy, yz, zz
 *               gradient a          ((t_a0*g_0) + t_a1*g_1) + t_a2*g_2,  t_ai = 0.5 * M[a][i]
 *   coeffs    xb_stencil_coeffs(lattice, nx, ny, nz, out): out[0..8] = t[3*a+i], out[9..14] = w_k, out[15..50] = h[6*ab+k].  Host only,
 *             needs no GPU.  XB_E_ARG: a null pointer, an axis below 1, a determinant that is exactly 0 or not finite.
 * The library is built without contraction, so every value above is the same bits wherever it is formed.  Every coefficient takes
 * part, zero ones included: an orthogonal cell has no definition of its own.  A constant field gives exactly 0.  An axis of one or
 * two voxels needs no special case: the wrapped neighbours coincide.  Second-order accuracy; a fourth-order stencil and any
 * smoothing of noisy data are out of scope.
 *   field     xb_laplacian_field: the Laplacian of every voxel, N doubles in C order, into out_host (host memory) or out_dev (device
 *             memory of the context's device that does not overlap the resident density) -- exactly one of the two is non-null.  The
 *             call returns when the result is written.
 *   sums      xb_laplacian_sum: over the voxels of every label a with 0 <= a < n (labels < 0 and >= n are skipped):  sum[a] = the sum
 *             of the Laplacian times voxel_volume (L of the basin),  abs_sum[a] = the sum of its magnitude times voxel_volume,
 *             volume[a] = the voxel count times voxel_volume.  The terms are bit-defined; the order of the sums is free (float
 *             atomics, as xb_charge_sum).  n <= 256 labels sum in LDS bins per block, more in global memory; waves that hold one
 *             label add once per wave.
 *   points    xb_stencil_points: for each of the m linear C-order indices lin[i] ten doubles out[10*i ..]: rho, the gradient x y z,
 *             the Hessian xx xy xz yy yz zz.  m == 0 writes nothing (lin and out may then be null).
 * XB_STENCIL_GATHER in `flags` (field and sums) reads the 19 values from global memory, one thread per voxel, instead of staging
 * 8 x 8 x 32 tiles with their halo in LDS: the second implementation, same bits for the field.
 * XB_E_STATE: no grid, no density (sums: no labels) on this grid yet, a context that holds a slab;  XB_E_ARG: a null pointer, both or
 * neither output of the field, unknown flag bits, n < 1, m < 0, an index outside [0, N), a lattice xb_stencil_coeffs refuses, a
 * device output that is not N doubles of device memory;  XB_E_LIMIT: n above 2^31 - 1.  No option key, no timer slot: a caller
 * times the calls.  The sums' device buffer (24 n bytes) is kept while the grid stays and counted by xb_memory_stats; the field
 * for a host output goes through the context's scratch. */
enum { XB_STENCIL_GATHER = 1 };
enum { XB_STENCIL_COEFFS = 51, XB_STENCIL_POINT_VALUES = 10 };
int xb_stencil_coeffs(const double lattice[9], int64_t nx, int64_t ny, int64_t nz, double out[XB_STENCIL_COEFFS]);
int xb_laplacian_field(xb_ctx *c, const double lattice[9], int flags, double *out_host, void *out_dev);
int xb_laplacian_sum(xb_ctx *c, const double lattice[9], int64_t n, double voxel_volume, int flags, double *sum, double *abs_sum,
                     double *volume);
int xb_stencil_points(xb_ctx *c, const double lattice[9], const int64_t *lin, int64_t m, double *out /* m*10 */);
/* ---- the NCI index (Johnson et al. 2010; what NCIPLOT, Multiwfn and Critic2 print): the reduced density gradient s and
 * sign(lambda2) rho at every voxel, the sums over the low-s, low-rho region per label split into attractive, van der Waals and
 * repulsive parts, and the s against sign(lambda2) rho histogram -- no counterpart in the reference ----
 * All three calls read the resident density rho of the whole grid (xb_nci_sum the resident labels too); nothing resident is
 * written.  lattice[9]: the cell, a row per axis.
 *   voxel     c = rho(p), the gradient g_x g_y g_z and the Hessian H_xx H_xy H_xz H_yy H_yz H_zz are EXACTLY the ten values of
 *             xb_stencil_points: the coefficients of xb_stencil_coeffs, the operations in the order written in the block above.
 *             Then, in this order:
 *               g2 = (gx*gx + gy*gy) + gz*gz
 *               I1 = (Hxx + Hyy) + Hzz
 *               I2 = ((Hxx*Hyy - Hxy*Hxy) + (Hxx*Hzz - Hxz*Hxz)) + (Hyy*Hzz - Hyz*Hyz)
 *               I3 = (Hxx*(Hyy*Hzz - Hyz*Hyz) - Hxy*(Hxy*Hzz - Hyz*Hxz)) + Hxz*(Hxy*Hyz - Hyy*Hxz)
 *   sigma     the sign of lambda2, the middle eigenvalue of H, without an eigen-solve.  The characteristic polynomial
 *             lambda^3 - I1 lambda^2 + I2 lambda - I3 of a symmetric matrix has real roots, so Descartes' rule is exact:
 *               p = the number of sign changes in (1, -I1, I2, -I3), zeros skipped;  z = the number of trailing zeros of that
 *               sequence;  neg = 3 - p - z;  sigma = +1 if p >= 2, -1 if neg >= 2, else 0.
 *             The computed invariants are taken as they are (a NaN counts as a zero); p + z <= 3 for any sequence, so sigma is an
 *             integer defined for every input.  A constant field gives 0.  Only the COUNT of signs enters: a rounding error in I3
 *             can flip sigma only where lambda2 itself is at rounding level.
 *   fields    where rho > 0:  x = sigma * rho (bit-defined),  s = sqrt(g2) / (C * (rho * cbrt(rho))),  C = XB_NCI_C = 2 (3 pi^2)^(1/3);
 *             where rho <= 0 (or NaN):  s = +inf, x = 0; such a voxel is in no region and no bin.  s is the only value here that is
 *             not bit-defined (sqrt and cbrt are library functions); nothing below uses it.
 *   s < e     for a threshold e on s the host forms  a = C*e,  a2 = a*a,  T(e) = (a2*a2)*a2;  per voxel  r2 = rho*rho,  r4 = r2*r2,
 *             r8 = r4*r4,  q = (g2*g2)*g2.  "s < e" MEANS  q < T(e)*r8:  multiplications and one comparison.  Denormal products take
 *             part as they are: nothing is flushed to zero.
 *   bins      edges e_0 < ... < e_m put a voxel into bin k = (the number of j with T(e_j)*r8 <= q) - 1; outside 0 .. m - 1 it is
 *             not counted.  (A binary search gives the same k: the products are monotone in T.)  x goes into its bins the same
 *             way, straight against its edges: k = (the number of j with xe_j <= x) - 1.
 *   region    rho > 0  and  s < s_cut (as above)  and  rho < rho_cut.  Its classes:  0 attractive, x < -rho_split;  1 van der Waals,
 *             -rho_split <= x <= rho_split;  2 repulsive, x > rho_split.  s is dimensionless when density and lattice share a length
 *             unit; rho_cut and rho_split are in the density's units.
 *   field     xb_nci_field: s and x of every voxel, N doubles each in C order, into s_host and x_host (host memory) or s_dev and
 *             x_dev (device memory of the context's device; neither overlaps the resident density or the other) -- either both
 *             host pointers or both device pointers are non-null.  The call returns when the result is written.
 *   sums      xb_nci_sum: over the voxels of the region that carry a label a with 0 <= a < n (labels < 0 and >= n are skipped), per
 *             key 3*a + class:  count[key] = the voxel count,  charge[key] = the sum of rho times voxel_volume,  charge2[key] = the
 *             sum of r2 = rho*rho times voxel_volume; 3 n entries each.  The terms are bit-defined; the order of the sums is free
 *             (float atomics, as xb_laplacian_sum).  n <= 85 labels (3 n <= 256 keys) sum in LDS bins per block, more in global
 *             memory; waves that hold one key add once per wave.
 *   hist      xb_nci_hist: counts[ks * n_x + kx] = the number of voxels with rho > 0 in bin ks of s_edges[0 .. n_s] and bin kx of
 *             x_edges[0 .. n_x]: exact integers.  n_s * n_x <= XB_NCI_HIST_LDS_BINS bins are counted in LDS per block, more in
 *             global memory.
 * XB_STENCIL_GATHER in `flags` reads the 19 values from global memory, one thread per voxel, instead of staging 8 x 8 x 32 tiles
 * with their halo in LDS: the second implementation of all three, same bits (s included: the same functions on the same bits).
 * XB_E_STATE: no grid, no density (sums: no labels) on this grid yet, a context that holds a slab;  XB_E_ARG: a null pointer, host
 * and device outputs of the field mixed or incomplete, unknown flag bits, n < 1, n_s < 1 or n_x < 1, a threshold (s_cut, rho_cut,
 * rho_split) that is not finite or negative, an edge that is not finite, s edges below 0, edges that do not increase strictly, a
 * lattice xb_stencil_coeffs refuses, a device output that is not N doubles of device memory;  XB_E_LIMIT: n above (2^31 - 1) / 3,
 * n_s, n_x or n_s * n_x above XB_NCI_BINS_MAX.  No option key, no timer slot: a caller times the calls.  The device buffer of the
 * sums (72 n bytes) and of the histogram (8 (n_s + n_x + 2 + n_s n_x) bytes) is one, kept while the grid stays and counted by
 * xb_memory_stats; the field for host outputs goes through the context's scratch and a temporary buffer of N doubles. */
#define XB_NCI_C 0x1.8bfd4dd6882cbp+2 /* 2 (3 pi^2)^(1/3) = 6.187335452560272, the nearest double */
enum { XB_NCI_ATTRACTIVE = 0, XB_NCI_VDW = 1, XB_NCI_REPULSIVE = 2, XB_NCI_CLASSES = 3 };
enum { XB_NCI_HIST_LDS_BINS = 1024, XB_NCI_BINS_MAX = 16777216 };
int xb_nci_field(xb_ctx *c, const double lattice[9], int flags, double *s_host, double *x_host, void *s_dev, void *x_dev);
int xb_nci_sum(xb_ctx *c, const double lattice[9], int64_t n, double voxel_volume, double s_cut, double rho_cut, double rho_split,
               int flags, int64_t *count, double *charge, double *charge2);
int xb_nci_hist(xb_ctx *c, const double lattice[9], const double *s_edges, int64_t n_s, const double *x_edges, int64_t n_x, int flags,
                int64_t *counts);
/* ---- DORI, the density overlap regions indicator (de Silva & Corminboeuf, J. Chem. Theory Comput. 10, 3745 (2014); what Multiwfn
 * prints): covalent and non-covalent overlap of the density in one field gamma on [0, 1], sign(lambda2) rho as its colour, and the
 * sums over the region gamma >= d_cut per label split into attractive, van der Waals and repulsive parts -- no counterpart in the
 * reference ----
 * Both calls read the resident density rho of the whole grid (xb_dori_sum the resident labels too); nothing resident is written.
 * lattice[9]: the cell, a row per axis.
 *   voxel     c = rho(p), the gradient g0 g1 g2 and the Hessian xx xy xz yy yz zz are EXACTLY the ten values of xb_stencil_points:
 *             the coefficients of xb_stencil_coeffs, the operations in the order written in the stencil block above.  Then, every
 *             line one IEEE float64 operation per operator, parenthesised as written:
 *               gg  = (g0*g0 + g1*g1) + g2*g2                                     (|grad rho|^2)
 *               h0  = (xx*g0 + xy*g1) + xz*g2
 *               h1  = (xy*g0 + yy*g1) + yz*g2
 *               h2  = (xz*g0 + yz*g1) + zz*g2                                     (H g)
 *               u_a = c*h_a - gg*g_a            (a = 0, 1, 2)                     (rho H g - |g|^2 g)
 *               N   = 4.0 * ((u0*u0 + u1*u1) + u2*u2)
 *               D   = (gg*gg)*gg
 *               S   = N + D
 *   gamma     = 0.0     if not (c > rho_min)                           (a NaN, +0, -0, a negative density: 0)
 *             = N / S   if S > 0 and S is finite
 *             = 1.0     if S == 0 and some component of the Hessian is not 0   (a critical point of the discrete field)
 *             = 0.0     otherwise                                      (a flat field, an overflow, a NaN)
 *             This is theta / (1 + theta) with theta = |grad k^2|^2 / (k^2)^3, k = grad rho / rho: grad k^2 = 2 u / rho^3 and
 *             (k^2)^3 = D / rho^6, so rho^6 cancels between numerator and denominator and no power of rho is formed.  No sqrt, no
 *             cbrt, no eigen-solve: gamma is bit-defined.  0 <= gamma <= 1 (S >= N by the monotony of rounding).  Range: N and D
 *             are of the sixth order in rho; a density scaled by 2^k gives the same bits while no product over- or underflows
 *             (|k| <= 100 on densities of order 1; not at |k| = 170), and so does a lattice scaled by 2^k.
 *   colour    x = sigma * c where c > rho_min, +0.0 elsewhere; sigma is the sign of lambda2 of the NCI block above (its I1, I2, I3
 *             and its Descartes rule).  With rho_min = 0 this is the x of xb_nci_field.
 *   region    gamma >= d_cut, decided on the value the field holds: field, sums, domains and surface agree by construction.  Its
 *             classes are those of the NCI block:  0 attractive, x < -rho_split;  1 van der Waals, -rho_split <= x <= rho_split;
 *             2 repulsive, x > rho_split.  gamma is dimensionless; rho_min and rho_split are in the density's units.
 *   field     xb_dori_field: gamma of every voxel, N doubles in C order, into g_host (host memory) or g_dev (device memory of the
 *             context's device) -- exactly one of the two is non-null -- and, if it is asked for, x into x_host or x_dev on the
 *             same side (null: gamma alone, and sigma is not formed).  A device output overlaps neither the resident density nor
 *             the other.  The call returns when the result is written.
 *   sums      xb_dori_sum: over the voxels of the region that carry a label a with 0 <= a < n (labels < 0 and >= n are skipped),
 *             per key 3*a + class:  count[key] = the voxel count,  charge[key] = the sum of rho times voxel_volume,  charge2[key]
 *             = the sum of rho*rho times voxel_volume; 3 n entries each.  The terms are bit-defined; the order of the sums is free
 *             (float atomics, as xb_nci_sum).  n <= 85 labels (3 n <= 256 keys) sum in LDS bins per block, more in global memory.
 * XB_STENCIL_GATHER in `flags` reads the 19 values from global memory, one thread per voxel, instead of staging 8 x 8 x 32 tiles
 * with their halo in LDS: the second implementation of both, same bits.
 * XB_E_STATE: no grid, no density (sums: no labels) on this grid yet, a context that holds a slab, host outputs while the context's
 * scratch buffer holds no whole grid;  XB_E_ARG: a null pointer, gamma on neither or on both sides, x on the other side, unknown
 * flag bits, n < 1, rho_min or rho_split not finite or negative, d_cut outside (0, 1], a lattice xb_stencil_coeffs refuses, a
 * device output that is not N doubles of device memory or overlaps the resident density or the other output;  XB_E_LIMIT: n above
 * (2^31 - 1) / 3.  No option key, no timer slot: a caller times the calls.  The sums use the device buffer of xb_nci_sum (72 n
 * bytes, kept while the grid stays and counted by xb_memory_stats); the field for host outputs goes through the context's scratch
 * and, with x, a temporary buffer of N doubles. */
int xb_dori_field(xb_ctx *c, const double lattice[9], double rho_min, int flags, double *g_host, double *x_host, void *g_dev,
                  void *x_dev);
int xb_dori_sum(xb_ctx *c, const double lattice[9], int64_t n, double voxel_volume, double d_cut, double rho_min, double rho_split,
                int flags, int64_t *count, double *charge, double *charge2);
/* ---- isosurfaces: marching tetrahedra on the Freudenthal (Kuhn) triangulation of the periodic voxel lattice (the 0.001 a.u.
 * molecular surface with its area and volume, in total and per atom; the zero envelopes of the Laplacian; the s = 0.5 surface of
 * the NCI index coloured by sign(lambda2) rho) -- no counterpart in the reference ----
 * Reads a field f of the whole grid -- the resident density (field_dev null) or N doubles of device memory in C order -- and, with
 * n_labels >= 1, the resident labels; nothing resident is written.  The triangulation is the one of the critical points above:
 * 6 tetrahedra per cube, no ambiguous case, crack-free across tiles and the periodic boundary; connectivity is integers.
 *   inside    inside(v) = f[v] >= level, a plain IEEE comparison: a NaN is outside, -0.0 and +0.0 are equal
 *   edges     voxel v owns the 7 lattice edges (v, k), k = 0 .. 6, towards v + d_k (the positive seven offsets of the critical
 *             points, every coordinate wrapped).  An edge CROSSES iff its two ends differ in inside().  The crossing edges are the
 *             vertices; the id of a vertex is the rank of 7 lin(v) + k among them, ascending
 *   vertex    a = f[v], b = f[v + d_k], t = (level - a) / (b - a): one division.  p_i = (double)v_i + (d_k,i ? t : 0), in voxel
 *             coordinates in the frame of its OWNER v.  One expression on the same two values, built without contraction: every
 *             triangle that uses the vertex sees the same bits.  With a colour field g (colour_dev, N doubles, or null):
 *             colour = g[v] + t * (g[v + d_k] - g[v])
 *   cube      cube v has the corners v + (cx, cy, cz), corner number 4 cx + 2 cy + cz.  Tetrahedron tau = 0 .. 5 is the path
 *             P_0 = 0 -> P_1 = e_a -> P_2 = e_a + e_b -> P_3 = (1, 1, 1) for (a, b, c) the tau-th permutation of (0, 1, 2) in
 *             lexicographic order; m = its inside bits (bit i: P_i).  Its edge P_lo P_hi (lo < hi) is the lattice edge
 *             (v + P_lo, k) with d_k = P_hi - P_lo
 *   triangles popcount(m) = 1 or 3: one triangle, on the three edges at the lone corner, the other ends ascending;  2 (inside i < j,
 *             outside k < l): the quadrilateral ik il jl jk split along ik -- jl into (ik, il, jl) and (ik, jl, jk);  0 or 4: none.
 *             The last two corners of a triangle are swapped where that makes its normal (q1 - q0) x (q2 - q0) in voxel
 *             coordinates point from the inside corners to the outside ones, so every mesh edge is traversed once in each direction.
 *             The triangles of the mesh ascend in (lin of the cube, tau, triangle within tau)
 *   table     xb_isosurface_table: out[(16 tau + m) 8 + 0] = the number of triangles, out[.. + 1 + 3 t + j] = corner j of triangle t
 *             as (owner corner of the cube) << 3 | k, 255 where unused; 768 bytes; host only, needs no GPU
 *   per tri   three vertex ids (int64);  wrap (uint16): bit 3 corner + axis is set iff that corner's owner lies across the periodic
 *             boundary from the cube along the axis -- the corner in the cube's frame is then vertex + n_axis;  cell (int64): lin of
 *             the cube
 *   area      the sum over the triangles of 0.5 sqrt((cx cx + cy cy) + cz cz), c = E1 x E2, E_j = (e_0 A[0][j] + e_1 A[1][j]) +
 *             e_2 A[2][j] for e = q1 - q0 and q2 - q0, the corners q in the cube's frame, A the voxel lattice of the Laplacian block
 *   volume    (|det A| / 6) times the sum over all tetrahedra of the inside fraction, det in the order of that block.  With u(a, b)
 *             the crossing's distance from corner a on the edge towards b (t where a < b, 1 - t otherwise):
 *               1 inside corner i, the others j < k < l:   (u(i,j) u(i,k)) u(i,l)
 *               3 inside, outside o, the others j < k < l:  1 - (u(o,j) u(o,k)) u(o,l)
 *               2 inside i < j, outside k < l:   (u(i,k) u(i,l) + (u(i,k) u(j,l)) (1 - u(i,l))) + (u(j,k) u(j,l)) (1 - u(i,k))
 *                                                (the wedge as the tetrahedra (P_i ik il P_j), (P_j ik il jl), (P_j ik jl jk))
 *               4: 1;  0: nothing
 *   labels    with n_labels >= 1, volume_by_label[a] = (|det A| / 6) times the sum of fraction / popcount(m) over every inside
 *             corner of every tetrahedron whose voxel carries label a (labels < 0 and >= n are skipped): a voxel whose 24
 *             tetrahedra are all inside gets one voxel volume, as in xb_charge_sum
 * The terms are bit-defined; the order of the sums is free (float atomics, as xb_laplacian_sum); LDS bins up to 256 labels.
 * Axes below 4: the definition stands as written (wrapped neighbours coincide); watertightness is not claimed there.
 * No smoothing, no vertex normals, no higher-order interpolation, no marching cubes.
 *   calls     xb_isosurface runs the passes (count; offsets and a scan in kernels of their own -- no kernel waits for another
 *             workgroup; emit) and keeps the mesh on the device: counts[0] = V, counts[1] = T.  It compares the emit pass's own
 *             counters with the count pass (XB_E_STATE on a mismatch); the emit pass never writes beyond the counted capacities.
 *             xb_isosurface_fetch copies into host arrays (on_device 0) or device arrays (on_device 1): vertices f64[3 V], colour
 *             f64[V] (null: not wanted), triangles i64[3 T], wrap u16[T], cell i64[T], scalars = {area, volume},
 *             volume_by_label f64[n_labels] (may be null when n_labels was 0).  It checks before it writes.
 *             xb_isosurface_release frees the mesh.  Any writer of the density discards the kept result.
 *   nci       xb_isosurface_nci_mask: s[v] = XB_ISO_NCI_RAISED wherever rho[v] >= rho_cut or s[v] is not below it (the +inf of a
 *             voxel without density, a NaN), in place on N doubles of device memory (what NCIPLOT does before it draws
 *             s = s_cut); rho is the resident density
 * XB_ISO_GATHER in `flags` reads the eight corners from global memory, one thread per voxel, instead of staging 8 x 8 x 32 tiles
 * with their halo in LDS: the second implementation, same results.
 * XB_E_STATE: no grid, no density, no labels with n_labels >= 1, a context that holds a slab (fetch: no result);  XB_E_ARG: a null
 * pointer, a field that is not N doubles of device memory or overlaps the scratch, field and colour overlapping without being one
 * array, unknown flag bits, a level that is not finite, n_labels < 0, a lattice xb_stencil_coeffs refuses, capacity below the
 * counts in a fetch, a colour asked of a mesh without;  XB_E_LIMIT: 7 N beyond the 64-bit range, n_labels above 2^31 - 1.  No
 * option key, no timer slot.  Memory: the per-voxel words and the scan live in the context's scratch (already counted); the kept
 * mesh is 24 V (+ 8 V with a colour) + 34 T bytes, each array at least one element, counted by xb_memory_stats.
 *   streams   xb_isosurface reads the caller's arrays on the context's stream.  A field or colour that another stream produces (a
 *             tensor made on a non-blocking stream) must be ordered first: xb_stream_wait(c, stream) makes the context's stream take
 *             up its work after everything queued on `stream` so far (an event, no host wait).  pybader_amd does so for every device
 *             field and colour it hands in.  xb_isosurface returns when the mesh is written: the caller may free its arrays then.
 * xb_device_write copies host bytes into device memory of the context's device (the counterpart of xb_device_read) and returns when
 * they are there.  The target is the caller's own memory: it must not be memory the context owns (the resident density handed out
 * by xb_density_ptr, the labels, the scratch) -- the call invalidates nothing. */
#define XB_ISO_NCI_RAISED 100.0
enum { XB_ISO_GATHER = 1 };
enum { XB_ISO_TABLE_SIZE = 768 };
int xb_isosurface_table(uint8_t *out);
int xb_isosurface(xb_ctx *c, const void *field_dev, const void *colour_dev, const double lattice[9], double level, int64_t n_labels,
                  int flags, int64_t counts[2]);
int xb_isosurface_fetch(xb_ctx *c, int on_device, void *vertices, void *colour, void *triangles, void *wrap, void *cell,
                        int64_t cap_vertices, int64_t cap_triangles, double scalars[2], double *volume_by_label, int64_t cap_labels);
int xb_isosurface_release(xb_ctx *c);
int xb_isosurface_nci_mask(xb_ctx *c, void *s_dev, double rho_cut);
int xb_stream_wait(xb_ctx *c, void *stream);
int xb_device_write(xb_ctx *c, void *dev_ptr, const void *src_host, int64_t bytes);
/* ---- connected regions: the components of a periodic voxel mask -- the islands of a level set, the pockets below it, the domains
 * of the NCI region -- each with its seed, size, top and integrals (what NCIPLOT's, Critic2's and Multiwfn's domain analyses start
 * from) -- no counterpart in the reference ----
 * The calls read the resident density rho of the whole grid, a caller's field and (the shares) the resident labels; nothing resident
 * is written, and the result can be computed while the labels stay resident.
 *   adjacency   lin is the C-order index.  The offsets are those of the critical points and the isosurface: d_0 .. d_6 = (0,0,1)
 *               (0,1,0) (0,1,1) (1,0,0) (1,0,1) (1,1,0) (1,1,1), d_{7+k} = -d_k.  u and v are adjacent iff u = wrap(v + d_k) for some k
 *               and u != v.  On an axis of length 1 a neighbour that wraps onto v itself counts for nothing; on an axis of length 2
 *               v + d and v - d are one voxel.  (1,-1,0) and its kin are NOT adjacent: the components of {field >= level} are the
 *               pieces the marching-tetrahedra surface of xb_isosurface encloses.
 *   members     XB_DOMAINS_ABOVE: field[v] >= level;  XB_DOMAINS_BELOW: field[v] < level -- field_dev (N doubles of device memory in C
 *               order), or the resident density when it is NULL;  XB_DOMAINS_NCI: the region of the NCI block above (rho > 0, s < s_cut
 *               as q < T(s_cut) r8, rho < rho_cut) on the resident density in the cell `lattice`, the operations of xb_nci_sum in their
 *               order; field_dev must be NULL.  A NaN is outside in every mode.
 *   components  those of the members under the adjacency.  A component's seed is its smallest lin; the components are numbered
 *               0 .. m - 1 in ascending seed.  map[v] (int32) is the component of v, -1 outside.  The numbering is unique: no output
 *               depends on a schedule.
 *   sums        xb_regions_sums, per component, on the RESIDENT density: seed;  count, its voxels;  top, its greatest voxel in the
 *               order of the critical points (key(rho), ties to the greater lin);  sum1 and sum2, the sums of rho and of rho*rho times
 *               voxel_volume.  With rho_split not NaN (components of the NCI region only) also count3, sum1_3, sum2_3 [3 m]: the same
 *               per class 3*i + k, the class of xb_nci_sum (x < -rho_split, between, x > rho_split); count is then the sum of the
 *               three counts and sum1, sum2 the three partial sums added in class order before the one multiplication.  The terms
 *               are bit-defined, the order of the sums is free (float atomics; a wave that holds one component adds once).
 *   shares      xb_regions_shares: the triplets (component, label, count) with count > 0 over the members whose resident label a has
 *               0 <= a < n, ascending in (component, label); xb_regions_shares_fetch copies them.  m * n <= XB_DOMAINS_SHARE_CELLS
 *               cells are counted in a dense table on the device (in LDS per workgroup up to 1024 cells) whose non-empty cells
 *               are compacted there; more, or XB_DOMAINS_SHARES_LIST in `flags`, lists the keys component * n + label of those
 *               voxels and sorts and counts them on the host: the same triplets.
 *   routes      the default labels 8 x 8 x 32 tiles by a union-find in LDS, joins the tiles' faces (the periodic wrap included) in
 *               global memory and flattens; XB_DOMAINS_GLOBAL joins every member with its seven forward neighbours in global memory:
 *               the second implementation, same map.  Both use one lock-free union that never waits for another wave: the roots are
 *               the smaller lin, atomicMin makes the link and its return value alone says whether it did.  XB_DOMAINS_GATHER (NCI
 *               mode) reads the predicate's 19 values from global memory instead of the staged tile, as XB_STENCIL_GATHER does.
 *   times       XB_DOMAINS_TIMES in `flags` puts an event on the stream before the first launch and behind each stage;
 *               xb_regions_times then gives the milliseconds of the last labelling: ms[0] membership and tile union-find (or
 *               parent[v] = v), ms[1] the unions across the faces (or all of them), ms[2] the flatten, ms[3] the numbering
 *               (its wait for the component count and the allocation of the seeds included).  XB_E_STATE without such a result.
 * The map (4 N bytes) and the seeds (4 m bytes) stay on the device until xb_regions_release, counted by xb_memory_stats;
 * xb_regions_fetch_map copies the map to host memory or, with on_device, to N int32 of device memory.  Every writer of the density
 * and every change of the grid discards the result.
 * XB_E_STATE: no grid, no density on this grid yet (shares: no labels), a context that holds a slab, sums, shares or a fetch without
 * a result, classes asked of components that are not the NCI region's;  XB_E_ARG: a null pointer, an unknown mode or flag bits, a
 * level that is NaN, a field in NCI mode, thresholds that are not finite or negative, a lattice xb_stencil_coeffs refuses, a field or
 * destination that is not N elements of device memory, a capacity below the length, n < 1;  XB_E_LIMIT: N above 2^31 - 1. */
enum { XB_DOMAINS_ABOVE = 0, XB_DOMAINS_BELOW = 1, XB_DOMAINS_NCI = 2 };
enum { XB_DOMAINS_GLOBAL = 1, XB_DOMAINS_SHARES_LIST = 2, XB_DOMAINS_GATHER = 4, XB_DOMAINS_TIMES = 8 };
enum { XB_DOMAINS_SHARE_CELLS = 16777216 };
int xb_regions_label(xb_ctx *c, int mode, const void *field_dev, double level, const double lattice[9], double s_cut, double rho_cut,
                     int flags, int64_t *m);
int xb_regions_sums(xb_ctx *c, double voxel_volume, double rho_split, int64_t *seed, int64_t *count, int64_t *top, double *sum1,
                    double *sum2, int64_t *count3, double *sum1_3, double *sum2_3, int64_t capacity);
int xb_regions_shares(xb_ctx *c, int64_t n, int flags, int64_t *n_triplets);
int xb_regions_shares_fetch(xb_ctx *c, int32_t *component, int32_t *label, int64_t *count, int64_t capacity);
int xb_regions_fetch_map(xb_ctx *c, int on_device, void *map);
int xb_regions_times(xb_ctx *c, double ms[4]);
int xb_regions_release(xb_ctx *c);
/* ---- Hirshfeld (stockholder) charges from radial pro-atom tables, the promolecular density and the deformation density (the charge
 * Critic2, Chargemol and Multiwfn print beside the Bader one: every voxel's density is shared among the atoms in proportion to what
 * each FREE atom would put there, w_a(r) = rho0_a(|r - R_a|) / sum_b rho0_b(|r - R_b|): no surfaces, no maxima, no sensitivity to
 * noise) -- no counterpart in the reference ----
 * xb_hirshfeld_setup puts the cell, the atoms and the pro-atoms on the device; xb_hirshfeld_sum and xb_hirshfeld_field read the
 * resident density of the whole grid and write nothing resident: not the density, not the labels, which they do not need at all.
 * All of it is IEEE float64 without contraction: every value at a voxel is bit-defined.
 *   pro-atoms S species; species s has a cutoff r_cut[s] > 0 and a table f[s][0..K] of K + 1 finite, non-negative doubles, K >= 1 the
 *             same for all (tables[s * (K + 1) + k]).  f[s][k] is the free-atom density at r^2 = k * r_cut[s]^2 / K: the table is
 *             uniform in r^2, so no square root enters a bit-defined value.  f[s][K] must be exactly 0: the interpolant reaches zero
 *             continuously at the cutoff, and dropping an image beyond the cutoff drops an exact zero.  The host computes
 *             rc2[s] = r_cut[s]*r_cut[s] and inv_h2[s] = K / rc2[s] once; these doubles are what the kernel uses.
 *   position  of voxel (p0, p1, p2), as xb_voronoi_assign's:  pc[j] = lat[j]*p0/nx;  pc[j] += lat[3+j]*p1/ny;  pc[j] += lat[6+j]*p2/nz
 *   image     (a, x, y, z) of atom a:  q[j] = atom[a][j] + ((lat[j]*x + lat[3+j]*y) + lat[6+j]*z);
 *             e[j] = pc[j] - q[j],  d2 = (e0*e0 + e1*e1) + e2*e2
 *   term      for an image of atom a with species s:  term = 0 when d2 >= rc2[s];  otherwise u = d2*inv_h2[s],
 *             k = min((int)u, K - 1),  t = u - k,  term = f[s][k] + t*(f[s][k+1] - f[s][k])
 *   list      the images (a, x, y, z) in CANONICAL ORDER: a ascending, then x, y, z ascending.  Per atom and axis i the shifts run over
 *             lo_i .. hi_i, which covers every image with any voxel of the cell closer than r_cut[species[a]].  With M the inverse
 *             of the lattice by cofactors, as xb_stencil_coeffs forms it with A = the lattice itself
 *               C[i][b] = A[i+1][b+1]*A[i+2][b+2] - A[i+1][b+2]*A[i+2][b+1],  det = (A[0][0]*C[0][0] + A[0][1]*C[0][1]) + A[0][2]*C[0][2],
 *               M[b][i] = C[i][b] / det                                         (indices mod 3)
 *             the atom's fractional coordinate, the reciprocal of the cell's height h_i = |det| / |a_j x a_k|, and the range are
 *               f_i  = (atom[a][0]*M[0][i] + atom[a][1]*M[1][i]) + atom[a][2]*M[2][i]
 *               g_i  = sqrt((M[0][i]*M[0][i] + M[1][i]*M[1][i]) + M[2][i]*M[2][i])            (= 1 / h_i)
 *               rho_i = r_cut[s]*g_i,   m_i = 2^-20 * ((1 + |f_i|) + rho_i)                    (the margin for the rounding of f and rho)
 *               lo_i = floor((-rho_i - f_i) - m_i),   hi_i = ceil(((1 + rho_i) - f_i) + m_i)
 *             Atoms are taken as given, not wrapped: an atom outside the cell only shifts its range.  A wider range adds zero terms
 *             only -- every term is >= +0 and x + 0.0 == x -- so NO RESULT DEPENDS ON THE RANGE.
 *   voxel     P(v) = the left-to-right running sum of all terms in list order;  p_a(v) = the same sum over atom a's images only,
 *             started from 0;  w_a = p_a / P,  term_a = rho(v) * w_a.  A voxel with P == 0 belongs to nobody.
 *   results   charge[a] = voxel_volume * sum_v term_a;  volume[a] = voxel_volume * sum_{v: P > 0} w_a;
 *             rest = {voxel_volume * sum_{v: P == 0} rho, voxel_volume * #{v: P == 0}};  the fields are P (XB_HIRSHFELD_PROMOLECULE)
 *             and rho - P (XB_HIRSHFELD_DEFORMATION), N doubles in C order.  The order of the sums over voxels is free (float
 *             atomics, as xb_charge_sum); everything per voxel is bit-defined.
 * xb_hirshfeld_images: HOST ONLY, needs no GPU.  Writes the canonical list (a, x, y, z as int32 quadruples) into out_images, which
 *             holds `capacity` quadruples, and its length into out_count; with out_images null only the length.
 * xb_hirshfeld_setup: species[n] in [0, n_species); tables[n_species * (knots + 1)]; knots = K.  Builds the list, q, the position
 *             table and the tables (as pairs f[k], f[k+1] - f[k]) in ONE device buffer of the context, grown on demand and counted by
 *             xb_memory_stats.  The setup belongs to the grid's SHAPE: it survives density and label uploads and every other call; an
 *             xb_set_grid that changes the shape drops it (the two calls below then answer XB_E_STATE); a call refused for its arguments
 *             leaves an earlier setup as it was, a new one replaces it; xb_hirshfeld_release frees it.
 * xb_hirshfeld_sum: charge[n], volume[n], rest[2] as above for the resident density (upload another, the spin, and call again: the
 *             setup is reused).  stats: NULL, or {tiles answered from a candidate list, tiles answered by the full search, the largest
 *             number of images a tile kept (it may exceed the cap; 0 with XB_HIRSHFELD_FULL_SEARCH)}.
 * xb_hirshfeld_field: mode XB_HIRSHFELD_PROMOLECULE or XB_HIRSHFELD_DEFORMATION into out_host (host memory) or out_dev (device memory
 *             of the context's device that overlaps neither the resident density nor the setup) -- exactly one of the two is
 *             non-null.  The promolecule reads no density: a context without one is accepted.
 * One workgroup per 8 x 8 x 8 tile of voxels.  It keeps the images within r_cut[s] + R + slack of the tile's centre (R the tile's
 * circumradius; csrc/k_cell.h derives the slack), compacts them IN LIST ORDER into LDS and lets every voxel run over those.  A
 * tile that keeps more than XB_HIRSHFELD_CAND_MAX images runs over the whole list from global memory; XB_HIRSHFELD_FULL_SEARCH in
 * `flags` makes every tile do so: the second implementation, for tests and benchmarks -- both give the same bits.
 * XB_E_STATE: no grid, no setup for this grid's shape, no density where it is read, a context that holds a slab;
 * XB_E_ARG: a null pointer (a null context included, in all five calls), n < 1, n_species < 1, knots < 1, a species index outside [0, n_species), a lattice entry or coordinate
 * that is not finite, a determinant that is exactly 0 (or not finite), r_cut not finite or <= 0, a table value that is negative or not
 * finite, f[s][K] != 0, unknown flag bits, an unknown mode, both or neither output of the field, a device output that is not N doubles
 * of device memory, a capacity below the list's length;  XB_E_LIMIT: an image list longer than 2^31 - 1 (or a shift beyond 2^30), more
 * than 2^26 table entries.  No option key, no timer slot: a caller times the calls.  Every error is found before any launch. */
enum { XB_HIRSHFELD_FULL_SEARCH = 1, XB_HIRSHFELD_CAND_MAX = 256 };
enum { XB_HIRSHFELD_PROMOLECULE = 0, XB_HIRSHFELD_DEFORMATION = 1 };
int xb_hirshfeld_images(const double lattice[9], const double *atoms_cart, const int32_t *species, int64_t n, const double *r_cut,
                        int64_t n_species, int64_t *out_count, int32_t *out_images, int64_t capacity);
int xb_hirshfeld_setup(xb_ctx *c, const double lattice[9], const double *atoms_cart, const int32_t *species, int64_t n,
                       const double *tables, const double *r_cut, int64_t n_species, int64_t knots);
int xb_hirshfeld_release(xb_ctx *c);
int xb_hirshfeld_sum(xb_ctx *c, double voxel_volume, int flags, double *charge, double *volume, double rest[2], int64_t stats[3]);
int xb_hirshfeld_field(xb_ctx *c, int mode, int flags, double *out_host, void *out_dev);
/* ---- Iterative stockholder atoms (ISA; Lillestolen & Wheatley 2008): Hirshfeld weights WITHOUT pro-atoms.  Each atom's table is the
 * spherical average of that atom's own share of the density, iterated to self-consistency; the charge HORTON and Chargemol print
 * beside the plain Hirshfeld one -- no counterpart in the reference ----
 * Everything not restated here is the Hirshfeld section's, bit for bit: voxel and image positions, d2, the canonical image list and
 * its margins, u = d2*inv_h2[a], k = min((int)u, K - 1), t = u - k, the running sums in list order, no contraction.
 *   tables    one per atom: species[a] = a, S = n; atom a has r_cut[a] > 0 and K >= 1 shells, the same K for all.  Shell k is
 *             k <= u < k + 1; because of the clamp the last shell also takes u up to the cutoff.
 *   weights   PIECEWISE CONSTANT: the term of an image of atom a at a voxel is A[a][k] when d2 < rc2[a], and 0 otherwise.  In the
 *             Hirshfeld section's table form this is the pair (A[a][k], +0.0), and f + t*0.0 == f: xb_hirshfeld_sum and
 *             xb_hirshfeld_field evaluate it with unchanged code and the same bits.
 *   counts    count[a][k] = the number of (voxel, image of a) pairs with d2 < rc2[a] that fall in shell k, int64.  Geometry only,
 *             computed once per setup; pairs at voxels with P == 0 count too.
 *   start     A0[a][k] = 1.0 for all shells, or the caller's [n][K] finite non-negative doubles.
 *   iteration for every voxel with P > 0 and every pair with term > 0:  c = rho*(term/P),  q = llrint(ldexp(c, e))  (to nearest,
 *             ties to even: numpy's rint),  bin[a][k] += q  in int64.  Integer addition is associative: the bins do not depend on
 *             the order of the atomics.  Then  A'[a][k] = bin > 0 ? ldexp((double)bin / (double)count, -e) : 0.0  -- a non-positive
 *             shell average (negative densities) clamps to zero.  The new tables replace the old, the bins are cleared, and
 *             qsum[a] = sum_k bin[a][k] (int64, wrapping) is kept per iteration: the atom's fixed-point charge, qsum * 2^-e *
 *             voxel_volume, for the convergence history.
 *   exponent  e = 61 - ceil_log2(rho_bound) - ceil_log2(cmax + 1), cmax = max count, formed with frexp and integers only; the
 *             caller's rho_bound >= max |rho|, finite, > 0.  |q| <= rho_bound*2^e (term <= P: a running sum of non-negative terms
 *             is monotone), so no bin can reach 2^62.  A voxel whose |rho| is not <= rho_bound adds nothing and is counted; any such
 *             voxel makes xb_isa_iterate fail with XB_E_ARG after the launch, and the tables stay as before the call.
 *   results   xb_hirshfeld_sum on the converged tables gives charge, volume and rest; xb_hirshfeld_field the sum of the atoms
 *             sum_a w_a and rho - sum_a w_a, the non-spherical residual: ISA's own quality figure.
 * On a uniform grid with piecewise-constant shells this is exactly an ML-EM iteration.
 * xb_isa_setup: builds the Hirshfeld setup of the context with these tables (it REPLACES an xb_hirshfeld_setup and the reverse; the
 *             stale-state rules are that call's), runs the counting pass and fixes e.  out_info = {e, cmax, the total number of
 *             pairs, the number of shells with count 0}.  initial: NULL or [n][K].
 * xb_isa_iterate: `iters` iterations (1 .. XB_ISA_ITERS_MAX) of the resident density queued back to back, ONE host wait; row i of
 *             qsum_out[iters][n] is iteration i's qsum.  flags: XB_HIRSHFELD_FULL_SEARCH (every tile runs over the whole list) and
 *             XB_ISA_DIRECT (one global atomic per pair instead of the waves' LDS windows): second implementations, the same bits.
 *             stats: NULL or {candidate tiles, full-search tiles, the longest list, voxels beyond rho_bound}.
 * xb_isa_tables: the current tables A_out[n][K] and the counts count_out[n][K]; either may be NULL, not both.
 * xb_isa_load: tables[n][K], finite and non-negative, replace the current tables of the setup (the counts and e stay): a caller
 *             goes back to tables it read earlier without a new setup.
 * xb_isa_rho_bound: max |rho| of the resident density (a NaN gives a NaN), for the rho_bound of a density that lives on the device.
 * XB_E_STATE: as the Hirshfeld calls, and xb_isa_iterate / xb_isa_tables / xb_isa_load on a setup that is xb_hirshfeld_setup's;  XB_E_ARG: as
 * xb_hirshfeld_setup, shells < 1, rho_bound not finite or <= 0, an initial value that is negative or not finite, iters < 1, unknown
 * flag bits, a density beyond rho_bound;  XB_E_LIMIT: as xb_hirshfeld_setup, n * shells above 2^26, iters above XB_ISA_ITERS_MAX.
 * Every argument error is found on the host before any launch. */
enum { XB_ISA_DIRECT = 2, XB_ISA_ITERS_MAX = 64 };
int xb_isa_setup(xb_ctx *c, const double lattice[9], const double *atoms_cart, int64_t n, const double *r_cut, int64_t shells,
                 const double *initial, double rho_bound, int64_t out_info[4]);
int xb_isa_iterate(xb_ctx *c, int64_t iters, int flags, int64_t *qsum_out, int64_t stats[4]);
int xb_isa_tables(xb_ctx *c, double *A_out, int64_t *count_out);
int xb_isa_load(xb_ctx *c, const double *tables);
int xb_isa_rho_bound(xb_ctx *c, double *out);
/* ---- Minimal-basis iterative stockholder atoms (MBIS; Verstraelen et al., JCTC 2016): iterative Hirshfeld weights whose pro-atoms
 * are sums of a few Slater shells, rho0_a(r) = sum_i N_ai / (8 pi sigma_ai^3) exp(-r / sigma_ai) -- 2 to 16 numbers of state per
 * atom instead of ISA's table; the charge HORTON, Psi4, Multiwfn and Chargemol print -- no counterpart in the reference ----
 * Everything not restated here is the Hirshfeld section's, bit for bit: voxel and image positions, d2, the canonical image list and its
 * margins (species[a] = a: r_cut and rc2 are per atom), the running sums in list order, IEEE float64 without contraction.  Double
 * sqrt and / are taken to be correctly rounded on the device.
 *   table     NO exp ON THE DEVICE.  The caller passes ONE table E[0..KE], E[k] = exp(-k / J) for k < KE (J knots per unit of
 *             x = r / sigma) and E[KE] = 0.0 exactly; finite, non-negative, J >= 1, 1 <= KE <= 2^26.  The library keeps the pairs
 *             (f[k], d[k]) = (E[k], E[k+1] - E[k]), the differences formed on the host.
 *   shells    shells[a] in 1 .. XB_MBIS_SHELLS_MAX; M = max_a shells[a] is the row stride of every [n][M] array (entries beyond an
 *             atom's own shells are not read; they come back as N = 0, sigma = 1).  Per shell, on the host at setup and load and in
 *             the update kernel alike:  den = ((EIGHT_PI*sigma)*sigma)*sigma,  c = (N > 0 && isfinite(N/den)) ? N/den : 0,
 *             is = 1.0/sigma,  EIGHT_PI the double 8.0 * M_PI.
 *   pair      (voxel, image of atom a) with d2 < rc2[a]:  r = sqrt(d2);  for i = 0 .. shells[a]-1:  u = (r*is_i)*(double)J,
 *             t_i = 0 when !(u < (double)KE), otherwise k = (int)u, w = u - k, t_i = c_i*(f[k] + w*d[k]).  The image's term is
 *             T = ((0 + t_0) + t_1) + ...;  P(v) = the left-to-right running sum of T in list order.
 *   iteration for every voxel with |rho| <= rho_bound and P > 0, and every pair: for each shell with t_i > 0
 *             s = rho*(t_i/P),  binN[a][i] += llrint(ldexp(s, eN)),  binS[a][i] += llrint(ldexp(r*s, eS));  with T > 0
 *             binV[a] += llrint(ldexp(T/P, eV)).  A voxel with !(P > 0) gives restq += llrint(ldexp(rho, eR)), restn += 1.  A voxel
 *             whose |rho| is not <= rho_bound adds nothing and is counted; any such voxel makes xb_mbis_iterate fail with XB_E_ARG
 *             after the launch, and the parameters stay as before the call.  All bins are int64: the order of the adds is free.
 *   exponents count[a] = the number of pairs with d2 < rc2[a] (a counting pass at setup), cmax = max count, cl2 = ceil_log2 by frexp
 *             and integers only:  eN = 61 - cl2(rho_bound) - cl2(cmax + 1),  eS = eN - max(0, cl2(max r_cut)),
 *             eV = 61 - cl2(cmax + 1),  eR = 61 - cl2(rho_bound) - cl2(N_vox + 1).  t_i <= T <= P (running sums of non-negative
 *             terms are monotone), so no bin reaches 2^62.
 *   update    per (a, i):  raw = ldexp((double)binN, -eN);  binN > 0:  N' = raw*voxel_volume,
 *             s1 = ldexp((double)binS, -eS) / (3.0*raw),  sigma' = (binS > 0 && s1 > 0 && isfinite(s1)) ? s1 : sigma;  otherwise
 *             N' = 0, sigma' = sigma: a dead shell stays dead.  Kept as a row per iteration: qsum[a] = sum_i binN[a][i] (int64),
 *             vsum[a] = binV[a], restq, restn.  The bins are cleared and the two parameter areas swapped.
 *   results   charge[a] = voxel_volume * ldexp((double)qsum[a], -eN) of the last iteration, volume[a] = voxel_volume *
 *             ldexp((double)vsum[a], -eV), rest = {voxel_volume * ldexp((double)restq, -eR), voxel_volume * restn}: exact, no extra pass.
 * xb_mbis_setup: builds the geometry of a Hirshfeld setup of the context (it REPLACES an xb_hirshfeld_setup or xb_isa_setup and the
 *             reverse), runs the counting pass and fixes the exponents.  init_N, init_sigma: [n][M], N finite and >= 0, sigma finite
 *             and > 0.  out_info = {eN, eS, eV, eR, cmax, the total number of pairs}.
 * xb_mbis_iterate: `iters` iterations (1 .. XB_MBIS_ITERS_MAX) of the resident density queued back to back, ONE host wait; row i of
 *             qsum_out[iters][n], vsum_out[iters][n] and rest_out[iters][2] = {restq, restn} is iteration i's.  flags:
 *             XB_HIRSHFELD_FULL_SEARCH (every tile runs over the whole list), XB_MBIS_DIRECT (one global integer atomic per pair and
 *             shell instead of the sums in registers, over the wave and in LDS): second implementations, the same bits;
 *             XB_MBIS_KEEP (iters == 1 only): the pass and its row, the parameters stay -- the spin density summed on converged
 *             weights.  stats: NULL or {candidate tiles, full-search tiles, the longest list, voxels beyond rho_bound}.
 * xb_mbis_params: the current N_out[n][M], sigma_out[n][M] and count_out[n]; each may be NULL, not all.
 * xb_mbis_load: N[n][M] and sigma[n][M], checked as at setup, replace the current parameters (the counts and exponents stay).
 * xb_mbis_field: sum_a rho0_a (XB_HIRSHFELD_PROMOLECULE) or rho minus it (XB_HIRSHFELD_DEFORMATION) of the current parameters; the
 *             destination rules are xb_hirshfeld_field's.
 * XB_E_STATE: as the Hirshfeld calls; xb_hirshfeld_sum, xb_hirshfeld_field and the xb_isa_* calls on an MBIS setup, the xb_mbis_* calls
 * on a setup of another kind;  XB_E_ARG: as xb_isa_setup, a shell count outside 1 .. 8, sigma not > 0, a population that is negative or
 * not finite, a bad table, voxel_volume not finite or <= 0, iters < 1, unknown flag bits, XB_MBIS_KEEP with iters != 1, a density
 * beyond rho_bound;  XB_E_LIMIT: as xb_hirshfeld_setup, KE above 2^26, n above 2^23, iters above XB_MBIS_ITERS_MAX.
 * Every argument error is found on the host before any launch. */
enum { XB_MBIS_DIRECT = 2, XB_MBIS_KEEP = 4, XB_MBIS_ITERS_MAX = 64, XB_MBIS_SHELLS_MAX = 8 };
int xb_mbis_setup(xb_ctx *c, const double lattice[9], const double *atoms_cart, int64_t n, const double *r_cut, const int32_t *shells,
                  const double *etable, int64_t J, int64_t KE, const double *init_N, const double *init_sigma, double rho_bound,
                  double voxel_volume, int64_t out_info[6]);
int xb_mbis_iterate(xb_ctx *c, int64_t iters, int flags, int64_t *qsum_out, int64_t *vsum_out, int64_t *rest_out, int64_t stats[4]);
int xb_mbis_params(xb_ctx *c, double *N_out, double *sigma_out, int64_t *count_out);
int xb_mbis_load(xb_ctx *c, const double *N, const double *sigma);
int xb_mbis_field(xb_ctx *c, int mode, int flags, double *out_host, void *out_dev);
/* ---- Stockholder atomic multipoles and radial moments: charge, dipole, second moments, <r^3> and <r^4> of every atom's share
 * w_a rho (what Psi4, HORTON and Multiwfn print after the stockholder charge; <r^3> / <r^3>_free is the Hirshfeld volume ratio of
 * the Tkatchenko-Scheffler correction).  xb_moment_sum needs a label map; a weight several atoms share at a voxel is none -- no
 * counterpart in the reference ----
 * One more pass over the (voxel, image) pairs of the setup that is current -- xb_hirshfeld_setup's, xb_isa_setup's or
 * xb_mbis_setup's -- on the resident density.  Everything not restated here is the Hirshfeld section's, bit for bit: the voxel
 * position pc, the image q and e[j] = pc[j] - q[j], d2 = (e0*e0 + e1*e1) + e2*e2, the canonical list with P(v) the running sum in
 * list order, IEEE float64 without contraction; double sqrt and / are taken to be correctly rounded on the device.
 *   term      T of an image at a voxel is the current setup's own: on a Hirshfeld or ISA setup the Hirshfeld section's term (the
 *             table uniform in r^2), on an MBIS setup that section's T = ((0 + t_0) + t_1) + ... with r = sqrt(d2) and the current
 *             parameters.
 *   pair      a voxel v and an image of atom a with  |rho(v)| <= rho_bound,  P(v) > 0,  d2 < rc2  and  T > 0.
 *   its terms left to right:  w = T / P,  s = rho * w,  r = sqrt(d2),  t_j = s * e[j],  u = s * d2
 *   bins      twelve int64 per atom, bins[a][0..11]:
 *               [0]      += llrint(ldexp(s, E0))
 *               [1 + j]  += llrint(ldexp(t_j, E1))                for j = 0, 1, 2
 *               [4 .. 9] += llrint(ldexp(t_j * e[k], E2))         for (j, k) = 00, 01, 02, 11, 12, 22: xb_moment_sum's columns
 *               [10]     += llrint(ldexp(u * r, E3))
 *               [11]     += llrint(ldexp(u * d2, E4))
 *             EACH IMAGE IS ITS OWN COPY OF THE ATOM: the displacement is the one to that image, not a minimum image, so an atom
 *             whose r_cut exceeds half the cell is summed consistently.  Integer addition is associative: the bins do not depend
 *             on the order of the atomics.
 *   exponents with frexp and integers only (cl2 = ceil_log2):  L = max(0, cl2(max r_cut)) over the setup's cutoffs;  count[a] = the
 *             number of (voxel, image of a) pairs with d2 < rc2, cmax = max_a count[a] -- ISA and MBIS setups hold the counts, a
 *             plain Hirshfeld setup gets them from one counting pass on its first moments call, kept with the setup;
 *               E_k = 61 - cl2(rho_bound) - cl2(cmax + 1) - k*L      for k = 0 .. 4
 *             NO BIN REACHES 2^62:  T <= P (running sums of non-negative terms are monotone), so w <= 1 and |s| <= rho_bound;
 *             |e_j| <= r < r_cut <= 2^L up to an ulp and d2 < rc2 <= 2^(2L) (1 + 2^-52), so a share of order k is below
 *             rho_bound 2^(k L) (1 + 2^-50) in magnitude and its integer below 2^(61 - cl2(cmax + 1)) (1 + 2^-50) + 1/2; at most
 *             cmax < 2^cl2(cmax + 1) of them meet in a bin: below 2^61 (1 + 2^-50) + cmax / 2 < 2^62.
 *   bound     a voxel whose |rho| is not <= rho_bound adds nothing and is counted; any such voxel makes the call fail with
 *             XB_E_ARG after the launch, and bins_out is then untouched (MBIS's rule).
 *   results   exact scalings:  moments[a][c] = voxel_volume * ldexp((double)bins[a][c], -E_order(c)),  order(c) = 0, 1 1 1,
 *             2 2 2 2 2 2, 3, 4.  Columns 0 .. 9 read exactly as a row of xb_moment_sum (m0; m1 x y z; m2 xx xy xz yy yz zz);
 *             columns 10 and 11 are the integrals of w_a rho r^3 and w_a rho r^4; <r^2> is the trace of the second moments.
 * xb_stockholder_moments: bins_out[n][12];  info = {E0, E1, E2, E3, E4, cmax, the total number of pairs with d2 < rc2, the voxels
 *             beyond rho_bound};  stats: NULL or xb_hirshfeld_sum's.  flags: XB_HIRSHFELD_FULL_SEARCH (every tile runs over the
 *             whole list) and XB_STOCKMOM_DIRECT (one global integer atomic per pair and bin instead of the sums in registers, over
 *             the wave and in LDS): second implementations, the same bits.  ONE host wait (a plain Hirshfeld setup's first call
 *             has one more, for its counts).  It writes nothing resident: not the density, not the tables, not the parameters;
 *             the bins of a call live in the buffer of xb_moment_sum, grown on demand and counted by xb_memory_stats.
 * XB_E_STATE: no grid, no setup for this grid's shape, no density, a context that holds a slab;  XB_E_ARG: a null pointer (a null
 * context included), rho_bound not finite or <= 0, unknown flag bits, a density beyond rho_bound.  Every error but the last is
 * found before any launch.  No option key, no timer slot: a caller times the call. */
enum { XB_STOCKMOM_DIRECT = 2 };
int xb_stockholder_moments(xb_ctx *c, double rho_bound, int flags, int64_t *bins_out /* n*12 */, int64_t info[8], int64_t stats[3]);
/* ---- IGM, the independent gradient model (Lefebvre et al., Phys. Chem. Chem. Phys. 19, 17928 (2017); the Hirshfeld-partitioned
 * IGMH of Lu and Chen, J. Comput. Chem. 43, 539 (2022); what IGMPlot and Multiwfn print): delta-g, the norm the density gradient
 * would have if the atomic gradients could not cancel minus the norm it has, and delta-g_inter, in which only the cancellation
 * BETWEEN user-named fragments counts -- no counterpart in the reference ----
 * xb_igm_field reads the current table setup (xb_hirshfeld_setup's or xb_isa_setup's, not xb_mbis_setup's) and the resident
 * density of the whole grid; nothing resident is written.  Everything not restated here is the Hirshfeld block's, bit for bit: pc,
 * q, e[j] = pc[j] - q[j], d2, rc2, ih2, the canonical image list, IEEE float64, no contraction.  Double sqrt and / are taken as
 * correctly rounded (the reliance of the stockholder moments).
 *   inputs    fragment[a], one int32 per atom of the setup, in -1 .. F-1 with 1 <= F <= 4 = XB_IGM_FRAGMENTS_MAX;  p_min >= 0;
 *             a mode, XB_IGM_PRO or XB_IGM_STOCKHOLDER.
 *   image     Per image i of atom a at voxel v: if d2 >= rc2 the image contributes nothing.  Otherwise, with k, t and the table
 *             pair (f, df) = (f[k], f[k+1] - f[k]) as in the Hirshfeld term:
 *               T    = f + t*df
 *               sl   = df * ih2
 *               c    = sl + sl
 *               G[j] = c * e[j]            (j = 0, 1, 2)
 *             G is the EXACT gradient of the table's own interpolant, which is linear in r^2: its slope is piecewise constant
 *             (it jumps at the knots; no smoothing is applied), and no square root is taken.
 *   sums      Running sums in list order:  P and gP[j] over all images;  p_a and gp_a[j] over atom a's images, started from 0.
 *   reached   A voxel is reached iff P > p_min.  At a voxel that is not reached both fields are +0.0.  The floor keeps 1/P finite:
 *             near the tables' cutoff P -> 0 while rho does not.
 *   atom      The atomic gradient ga[j] exists only for an atom with fragment[a] >= 0 and p_a > 0:
 *               XB_IGM_PRO           ga[j] = gp_a[j]
 *               XB_IGM_STOCKHOLDER   iP = 1.0 / P
 *                                    w  = p_a * iP
 *                                    ga[j] = w * gr[j] + rho * ((gp_a[j] - w * gP[j]) * iP)
 *             gr is the gradient of the resident density rho at v: values 1..3 of xb_stencil_points.  Atoms with fragment[a] == -1
 *             enter P and gP only.
 *   total     Atoms ascending:  g[j] += ga[j];  gI[j] += fabs(ga[j]);  gF[fragment[a]][j] += ga[j].  Then
 *               gX[j]  = ((|gF[0][j]| + |gF[1][j]|) + ...) over the F fragments
 *               nrm(v) = sqrt((v0*v0 + v1*v1) + v2*v2)
 *   fields    dg  = nrm(gI) - nrm(g)          (delta-g)
 *             dgi = nrm(gX) - nrm(g)          (delta-g_inter)
 *             Neither is clamped: mathematically 0 <= dgi <= dg, rounding gives values a few 1e-15 below 0.  delta-g_intra =
 *             dg - dgi is the caller's subtraction.  An image beyond its cutoff and an atom with p_a == 0 add nothing, so no bit
 *             depends on the image range or on the route a tile takes.
 * xb_igm_field: dg into dg_host (host memory) or dg_dev (device memory of the context's device) or nowhere (both null), dgi
 *             likewise; at least one of the four is non-null; N doubles in C order each.  lattice[9] is the setup's (the gradient
 *             of rho needs it).  flags: XB_HIRSHFELD_FULL_SEARCH (every tile runs over the whole list; the same bits).  stats:
 *             NULL or xb_hirshfeld_sum's.  The call returns when the results are written.
 * xb_igm_sum: one pass over the resident density rho, the resident labels and two fields of N doubles in device memory, val and
 *             x.  Over the voxels with val >= cut (decided on the STORED value, so that field, sums, domains and surface agree)
 *             that carry a label a with 0 <= a < n, per key 3*a + class (0: x < -rho_split;  2: x > rho_split;  1: otherwise):
 *             count[key] = the voxel count,  charge[key] = the sum of rho times voxel_volume,  integral[key] = the sum of val
 *             times voxel_volume; 3 n entries each.  The order of the sums is free (float atomics, as xb_nci_sum).
 * XB_E_STATE: no grid, no table setup for this grid's shape, an MBIS setup current, no density (sums: no labels), a context that
 * holds a slab, host outputs while the context's scratch buffer holds no whole grid;  XB_E_ARG: a null context (field), a null
 * pointer, fragment[a] outside -1 .. n_fragments-1, n_fragments outside 1 .. 4, an unknown mode, unknown flag bits, p_min negative
 * or not finite, a lattice xb_stencil_coeffs refuses or other than the setup's, a field asked for on both sides or none asked
 * for, a device array that is not N doubles of device memory, an output that overlaps the resident density, the setup, the
 * context's buffers or the other output; n < 1, rho_split negative or not finite, cut not above 0 or not finite;  XB_E_LIMIT: n
 * above (2^31 - 1) / 3.  Every error is found before any launch.  No option key, no timer slot: a caller times the calls.  Both use
 * the device buffer of xb_nci_sum (8 + 4 n bytes for the field, 72 n for the sums; counted by xb_memory_stats); host outputs go
 * through the context's scratch and, when both fields go to the host, a temporary buffer of N doubles. */
enum { XB_IGM_PRO = 0, XB_IGM_STOCKHOLDER = 1, XB_IGM_FRAGMENTS_MAX = 4 };
int xb_igm_field(xb_ctx *c, const double lattice[9], const int32_t *fragment /* n */, int n_fragments, int mode, double p_min, int flags,
                 double *dg_host, double *dgi_host, void *dg_dev, void *dgi_dev, int64_t stats[3]);
int xb_igm_sum(xb_ctx *c, const void *val_dev, const void *x_dev, int64_t n, double voxel_volume, double cut, double rho_split,
               int64_t *count /* n*3 */, double *charge, double *integral);
/* utils.volume_assign (utils.py:404-421): labels[v] = swap[labels[v]] for labels >= 0 */
int xb_volume_assign(xb_ctx *c, const int64_t *swap, int64_t n_swap);
/* utils.atom_assign (utils.py:185-232): nearest atom of every maximum over the 27 periodic images (one
 * device thread per maximum; context free: buffers on the current device) */
int xb_atom_assign(const double *bader_max_cart, int64_t n_max, const double *atoms_cart, int64_t n_atoms,
                   const double lattice[9], int64_t *atom_out, double *dist_out);

/* thread_handlers.surface_distance (thread_handlers.py:239-297) + utils.surface_dist (utils.py:320-379)
 * on the resident atom map (labels = atoms_volumes): runs edge_find, then returns per atom the minimum
 * SQUARED distance of its edge voxels to the atom over the 27 periodic images (+inf: no edge voxel). */
int xb_surface_distance(xb_ctx *c, const double lattice[9], const double *atoms_cart, int64_t n_atoms,
                        double *min_d2, int64_t *edges);
/* utils.volume_mask (utils.py:461-476): density where labels == vol_num, else 0 (host float64 N) */
int xb_volume_mask(xb_ctx *c, int64_t vol_num, double *out_host);
/* sum of the resident density / count over owned voxels with labels == value (vacuum sums when the
 * reference density differs from the charge density, utils.py:396-400) */
int xb_label_sum(xb_ctx *c, int64_t value, double *sum, int64_t *count);

/* ---- windowed table build (multi-GPU): each rank builds the 32-B/voxel gradient-field table only for
 * its slab +- `margin` planes.  The trapping regions need two global inputs, exchanged by the slab
 * scheduler between the two calls: the 26-neighbour maxima of every rank (tiny) and the per-brick move
 * masks (one int per 8^3 brick; every rank contributes the bricks of its own slab).
 *   xb_set_table_window -> xb_table_build -> [all-gather seeds + masks] -> xb_table_finish -> xb_assign_trace */
int xb_set_table_window(xb_ctx *c, int64_t margin);           /* margin < 0: whole grid (default) */
int xb_table_build(xb_ctx *c, int64_t *n_local_seeds);
int xb_table_local_seeds(xb_ctx *c, int64_t *out, int64_t capacity);  /* linear voxel indices */
int xb_brick_masks(xb_ctx *c, void **dev_ptr, int64_t *n_bricks, int64_t *own_first, int64_t *own_count);
/* does this rank's window hold a voxel whose record depends on the tie rule (methods.py:324 vs refinement.py:111)? */
int xb_table_ties(xb_ctx *c, int64_t *has_ties);
/* any_ties: the OR of xb_table_ties over all ranks */
int xb_table_finish(xb_ctx *c, const int64_t *seeds, int64_t n_seeds, int64_t any_ties);

/* ---- slab halo planes (multi-GPU) -------------------------------------------------------- */
/* Device pointers of the label / known arrays and the plane size in elements, so that the slab
 * scheduler can hand plane ranges to RCCL (ncclSend/ncclRecv) or any other transport.  On a slab, writes through
 * the label pointer must stay within the planes [x0 - halo, x1 + halo): the library keeps the rest zero.
 * The library does not see what is written through xb_labels_ptr / xb_density_ptr: keeping its cached state in step with such
 * writes is the caller's responsibility (write whole planes with xb_copy_planes or voxels with xb_scatter_voxels where that matters). */
void *xb_labels_ptr(xb_ctx *c);
void *xb_known_ptr(xb_ctx *c);
void *xb_density_ptr(xb_ctx *c);
int64_t xb_plane_elems(xb_ctx *c);
/* copy whole x-planes [xa,xb) of labels/known between host and device (halo transport over the
 * host / gloo; the RCCL transport works on the device pointers above).  Label planes copied to the device invalidate the
 * edge and changed-voxel lists and xb_vacuum_assign's promise about the -1 labels, as xb_scatter_voxels does.  On a context that
 * holds the whole grid they also drop the per-brick label marks, and the next assignment treats the grid as one with vacuum
 * whether the planes hold a -1 or not; on a slab the planes are taken to be halo planes of peers that ran the same assignment
 * (the regions' labels stay; a negative label still brings the vacuum back).  Planes of `known` drop the lists and the
 * uniformity marks.  Copies to the host invalidate nothing. */
int xb_copy_planes(xb_ctx *c, int which /*0 labels,1 known*/, int to_device, void *host, int64_t xa, int64_t xb);
/* Bytes per label (1 / 2 / 4) a label halo travels in (xb_comm_exchange_planes): the narrowest signed width that holds every
 * resident label -- the reference's own dtype_calc(-n_maxima) (thread_handlers.py:70-74, utils.py:25-37).  Sender and
 * receiver must agree on it.  It changes only in calls all ranks make alike (numbering, xb_upload_labels,
 * xb_vacuum_assign, xb_volume_assign); xb_scatter_voxels / xb_copy_planes widen it only when a label they write does not fit.
 * widen_to 1 / 2 / 4 raises it (0: only ask): after a per-rank write a scheduler sets the maximum over the ranks. */
int xb_label_wire(xb_ctx *c, int widen_to, int *wire_out);
/* the chunk [first, first+count) of the per-brick move masks (xb_brick_masks) and of the bricks' single-maximum voxels
 * (2 * count ints: masks, then voxels) from (to_device 1) or to (0) host memory -- the host-staged fallback of xb_comm_share_brick_masks */
int xb_brick_masks_copy(xb_ctx *c, int to_device, int32_t *host, int64_t first, int64_t count);
int xb_set_halo(xb_ctx *c, int64_t halo); /* planes each side of [x0,x1) that hold valid neighbour data */

/* ---- the slab step with its control flow on the device (csrc/slab_step.h) ------------------------------------
 * The same work as xb_table_build .. xb_assign_finish and xb_edge_find + xb_refine_trace above (thread_handlers.py:28-75,
 * 128-236 across slabs), but no list length, counter or table goes through the host between the launches: TWO host waits
 * per assignment + refinement pass instead of about fifteen.  Between the calls the scheduler (pybader_amd/slab.py) runs the
 * exchanges on device "blocks" (xb_slab_block): 0-2 the brick arrays of pass A, 3 the ranks' tie flags, 4 their maxima
 * tables, 6 / 7 the walkers of a refinement pass (all gathered: xb_comm_allgather_block), 5 the counters of a refinement
 * pass (summed: xb_comm_allreduce_block).
 *   xb_slab_assign_masks -> [blocks 0-3] -> xb_slab_assign_trace -> [block 4] -> xb_slab_assign_finish (waits)
 *   [label halos] -> xb_slab_refine_pass -> { [block 6 / 7] -> xb_slab_walkers_round } -> [block 5] -> xb_slab_refine_counts (waits)
 * xb_slab_supported: whole-brick slabs with a table window, no vacuum, at most 64 ranks.  xb_slab_assign_finish status:
 * 0 done, 1 repeat the step (the region growth wants its long schedule; every rank sees the same verdict), 2 use the
 * host-driven calls for this density (a rank has more than 1024 maxima or trajectories for the exact slow kernel). */
int xb_slab_supported(xb_ctx *c, int nranks, int64_t *ok);
int xb_slab_assign_masks(xb_ctx *c, int rank, int nranks);
int xb_slab_assign_trace(xb_ctx *c);
int xb_slab_assign_finish(xb_ctx *c, int64_t *n_maxima, int64_t *status);
int xb_slab_refine_pass(xb_ctx *c);
/* the walkers of the pass (retraces that left this rank's valid planes) travel in blocks 6 / 7, alternately: after block
 * 6 + src was gathered, its results are applied and -- unless `last` -- its walkers that arrive on this rank's planes are
 * carried on into this rank's part of the other block.  The last round packs the counters into block 5. */
int xb_slab_walkers_round(xb_ctx *c, int src, int last);
/* what travels of a rank's part of blocks 6 / 7 (fixed sizes: no count goes through the host): [0] bytes of a part,
 * [1] header + walkers of the pass itself, [2] header + walkers of a later round, [3] offset and [4] bytes of the results */
int xb_slab_walk_layout(xb_ctx *c, int64_t out[5]);
/* (round 5) how many walkers of a rank's part travel in the gather of the NEXT passes (0: the part's capacity).  The scheduler sets it
 * on every rank to the same value -- a bound on any rank's share it knows from the previous pass's summed export count -- and asks
 * xb_slab_walk_layout again; a rank that exports more loses the surplus to the host-driven path queries, as with a full part.
 * Replaces nothing in the reference (its threads share memory, thread_handlers.py:154-232). */
int xb_slab_walk_send(xb_ctx *c, int64_t walkers);
/* the int64 entries of block 5 and of local[] / global[] below (pybader_amd/_lib.py mirrors them) */
enum {
    XB_XC_EDGES = 0,      /* edge voxels of the sweep */
    XB_XC_CHANGED = 1,    /* voxels relabelled, by retraces and by applied walker results */
    XB_XC_ESCAPED = 2,    /* retraces that left their rank's valid planes (exported as walkers or parked) */
    XB_XC_TRAVELLING = 3, /* walkers still travelling after the last round: all ranks' already, so global[] holds nranks times it */
    XB_XC_SLOW = 4,       /* retraces for the exact slow kernel: xb_slab_refine_counts runs them, local[XB_XC_CHANGED] and
                           * local[XB_XC_ESCAPED] are the counts after it and the caller sums once more */
    XB_XC_LOST = 5,       /* walkers or results lost to a full block, or stuck (their voxels stay parked: xb_escaped_paths) */
    XB_XC_MINE = 6,       /* this rank's travelling walkers (xb_walkers_fetch) */
    XB_XC_ROUNDS = 7,     /* byte k (k < 4) != 0: this rank carried walkers on in round k; summed: how many ranks did -- the
                           * scheduler sizes the next pass's rounds by it */
    XB_XC_COUNT = 8
};
/* local[XB_XC_COUNT]: this rank's entries; global[XB_XC_COUNT]: their sums over the ranks */
int xb_slab_refine_counts(xb_ctx *c, int64_t *local, int64_t *global);
int xb_slab_block(xb_ctx *c, int which, void **dev_ptr, int64_t *bytes_total, int64_t *own_offset, int64_t *own_bytes);
/* bytes [off, off + bytes) of a block from (to_device 1) or to (0) host memory: the host-staged transports */
int xb_slab_block_copy(xb_ctx *c, int which, int to_device, void *host, int64_t off, int64_t bytes);
/* waits of the host for the card inside library calls made by the calling thread since it started */
int xb_host_waits(int64_t *n);

/* ---- measurement ------------------------------------------------------------------------- */
/* The numbered vocabulary below (timer slots, option keys, their values and bits) is FROZEN: benchmarks and tools pass the values
 * as plain integers, so a name may be added but no value changes or is used again.  pybader_amd/_lib.py mirrors every name. */
/* `which` of xb_kernel_time, and the bit (k + 1) of xb_enable_timing's mask */
enum {
    XB_TIMER_ASSIGN = 0,        /* the neargrid assignment after pass A: walk list, records, walker trace */
    XB_TIMER_OG_MASKS = 1,      /* the ongrid pointer pass (k_og_masks) */
    XB_TIMER_EDGE_FIND = 2,     /* edge_find */
    XB_TIMER_REFINE_TRACE = 3,  /* the refinement's retraces */
    XB_TIMER_MASKS_GROWTH = 4,  /* pass A + region growth (and records built for a refinement) */
    XB_TIMER_BRICK_MASKS = 5,   /* k_brick_masks alone */
    XB_TIMER_TRACE = 6,         /* the trace kernel alone */
    XB_TIMER_BRICK_RECORDS = 7, /* k_brick_records alone */
    XB_TIMER_MOMENTS = 8,       /* the kernels of xb_moment_sum */
    XB_TIMER_ADJACENCY = 9,     /* the kernels of xb_adjacency: one interval per group of launches between two host waits */
    XB_TIMER_MERGE = 10,        /* the kernels of xb_merge_basins, likewise: the initialisation, each round's two passes and decision,
                                 * each round's pointer doubling */
    XB_TIMER_COUNT = 11
};
/* HIP-event timing of the stages, measured on the context's stream: accumulated milliseconds and launch count of timer `which`
 * (XB_TIMER_*) since the last reset.  XB_E_ARG: `which` outside [0, XB_TIMER_COUNT). */
int xb_kernel_time(xb_ctx *c, int which, double *ms_total, int64_t *launches);
int xb_kernel_time_reset(xb_ctx *c);
/* on: 0 off, 1 every timer, otherwise a mask: bit k + 1 switches timer `which` = k on (event pairs between dependent kernels
 * cost stream time: a benchmark keeps only the dominant kernel's timer on inside its timed region) */
int xb_enable_timing(xb_ctx *c, int on);
/* `key` of xb_set_option */
enum {
    XB_OPT_REGIONS = 1,           /* XB_REGIONS_* bits; without both of them: plain full trajectories from a record per voxel -- the
                                   * exactness cross-check of the whole design */
    XB_OPT_CROSS_CHECK = 2,       /* XB_CHECK_* bits, each selecting the second implementation of one step so that a test can compare
                                   * the two */
    XB_OPT_DEBUG = 3,             /* XB_DBG_* bits */
    XB_OPT_EC_GROUPS = 4,         /* test plumbing: workgroups of the edge_check chase, 1..4096 (default 256) ... */
    XB_OPT_EC_QCAP = 5,           /* ... and its LDS queue capacity, from 2 up to the default (lowered to force the overflow hand-over) */
    XB_OPT_DROP_TABLE = 6,        /* drop the cached gradient-field table (benchmarks: a table kept from an earlier step would hide
                                   * 1.6 ms per step); the value is not kept, see XB_DROP_TABLE_AND_MAXIMA */
    XB_OPT_KILL_LAUNCHES = 17,    /* test plumbing: kill launches scheduled after a chase, >= 1 (default 6; 1 forces the repeat) */
    XB_OPT_SELF_EXCHANGE = 19,    /* test plumbing: a rank may exchange planes with itself */
    XB_OPT_ASYNC_COMM = 24,       /* collectives return without waiting (set by pybader_amd.slab itself) */
    XB_OPT_WEIGHT_NO_LABELS = 30  /* xb_weight_sum ignores the resident labels (1: no voxel is vacuum, the labels are not read;
                                   * pybader_amd.weight sets it for a call without a label map and clears it again) -- the one switch
                                   * that selects an input rather than an implementation */
};
/* value of XB_OPT_REGIONS: both bits by default.  Trapping regions are built, per 8^3 brick, only with BOTH bits set; one bit alone
 * selects the same plain path as 0 */
enum {
    XB_REGIONS_BOXES = 1,
    XB_REGIONS_BRICKS = 2
};
/* value of XB_OPT_DROP_TABLE that also forgets which bricks hold a 26-neighbour maximum (any other value keeps that) */
enum { XB_DROP_TABLE_AND_MAXIMA = 2 };
/* value of XB_OPT_CROSS_CHECK: a set bit selects the second implementation */
enum {
    XB_CHECK_NO_MIRROR = 1,       /* pass A runs the exact ongrid plane test for every open face (no mirror prefilter) */
    XB_CHECK_GENERIC_WALKER = 2,  /* the generic walker instead of the lean one */
    XB_CHECK_FULL_TGRAD = 4,      /* the full T_grad . grad product on orthogonal lattices too */
    XB_CHECK_LIST_DILATE = 8,     /* the dilation of the edge sweep from the edge list instead of tile by tile */
    XB_CHECK_WIDE_HALO = 16,      /* label halos travel as int32 */
    XB_CHECK_NO_EC_SHARE = 32,    /* no front sharing in the edge_check chase: every workgroup keeps what it wakes */
    XB_CHECK_IO_GATHER = 64       /* xb_import_density gathers a permuted layout voxel by voxel instead of through the LDS tile */
};
/* One more bit of the same value: the lean walker and the lean retrace ask the brick label / brick byte on every step instead of
 * reading the neighbour bits of the record in hand.  A macro, not an enumerator: tests/test_abi_cpu.py pins the enumerators above
 * and their number (pybader_amd._lib mirrors it as CROSS_CHECK_BRICK_LOOKUP). */
#define XB_CHECK_BRICK_LOOKUP 128
/* ... and one more: the edge sweep of the listed tiles voxel by voxel (k_edge_flag_listed) with the dilation in a kernel of its
 * own, instead of by row bit masks with the dilation fused in (k_edge_sweep_bits).  CROSS_CHECK_VOXEL_SWEEP in pybader_amd._lib. */
#define XB_CHECK_VOXEL_SWEEP 256
/* ... and one more: the generic retrace kernel (k_refine_trace) where the lean retrace of one GPU (k_refine_trace_lean: a whole-grid
 * table of whole bricks with valid neighbour bits, the labels of the last neargrid assignment, no vacuum, at most 2^27 voxels) would
 * run.  CROSS_CHECK_GENERIC_RETRACE in pybader_amd._lib. */
#define XB_CHECK_GENERIC_RETRACE 512
/* value of XB_OPT_DEBUG (bits 1, 2 and 8 are not in use) */
enum {
    XB_DBG_EC_PASSES = 4,         /* print the passes of edge_check and what the middle tier leaves for the exact slow kernel */
    XB_DBG_SLAB_STATS = 16,       /* print the statistics of the device-driven slab step */
    XB_DBG_STAGE_WAIT = 32,       /* wait after every stage of an assignment and say so */
    XB_DBG_SHORT_TIERS = 64       /* the exact slow path with tiers of 3 / 5 / 8 path voxels, so that a test reaches its last tier */
};
/* One more bit of the same value, a macro like XB_CHECK_BRICK_LOOKUP (tests/test_abi_cpu.py pins the enumerators above): the voxels
 * the first retrace of every edge list puts on its overflow list are kept on the host for xb_retrace_overflow
 * (DEBUG_KEEP_RETRACE_OVERFLOW in pybader_amd._lib). */
#define XB_DBG_KEEP_RETRACE_OVERFLOW 128
/* Switches.  A USER of the library sets none of them: every default is the measured best, and no switch but
 * XB_OPT_WEIGHT_NO_LABELS changes a result.  A key that is not an XB_OPT_* value, or a value outside the range its key states, is
 * XB_E_ARG.  (Round 4 removed keys 0, 2, 9-12, 15, 21; round 6 removed 7, 8, 16, 22 -- routes and launch shapes nobody set -- and
 * folded 13, 14, 18, 20, 25, 29 into the bits of XB_OPT_CROSS_CHECK.) */
int xb_set_option(xb_ctx *c, int key, int value);
/* device bytes held for the grid (density, labels, flags, numbering + the table of the window planes + scratch sized by the
 * slab): what a rank of the slab decomposition costs; the reference's blocks are copies of the block extent
 * (thread_handlers.py:31-47, utils.py:424-458) */
/* Page-locked host buffers for result arrays (no counterpart in the reference: numpy allocates its own).  A device-to-host
 * copy into such a buffer is one DMA transfer; into pageable memory it is staged through the library's pinned chunks and copied
 * again.  pybader_amd._lib hands out the narrowed label arrays of bader_calc (thread_handlers.py:70-74) from a pool of these. */
int xb_host_alloc(int64_t bytes, void **out);
int xb_host_free(void *p);
int xb_memory_stats(xb_ctx *c, int64_t *bytes_total, int64_t *bytes_table, int64_t *bytes_scratch);
/* statistics of the last assignment: trapping boxes found and voxels they cover */
int xb_box_stats(xb_ctx *c, int64_t *n_boxes, int64_t *box_voxels);
/* The brick lattice of the last neargrid assignment and, per 8^3 brick (C order over dims), the trapping region it was
 * certified for (> 0), 0 (its voxels were walked) or INT32_MIN (round 6: with a vacuum tolerance, a brick whose largest
 * density lies below it -- nothing to assign, no records).  dims = ceil(shape / 8): a brick the grid cuts holds the voxels the
 * grid leaves of it.  A diagnostic of the library's own decomposition (the reference has no counterpart); capacity in ints. */
int xb_brick_labels(xb_ctx *c, int32_t *out, int64_t capacity, int64_t dims[3]);
/* trajectories / retraces handed to the exact slow kernel since the context was created */
int xb_slow_path_stats(xb_ctx *c, int64_t *assign_total, int64_t *refine_total);
/* retraces redone by the from-rho kernel since the context was created (their walk went on through a brick whose
 * records the sparse table does not hold) */
int xb_deferred_stats(xb_ctx *c, int64_t *refine_total);
/* edge sweeps launched since the context was created: by row bit masks (no vacuum, the whole grid, whole 4 x 8 x 64 tiles and
 * at least 16 x 16 x 80 voxels, no table whose brick bytes flag every brick as a possible maximum's, fewer maxima in the last assignment than one per 8 bricks), and by the per-voxel kernels
 * (everything else, and everything under XB_CHECK_VOXEL_SWEEP) */
int xb_sweep_stats(xb_ctx *c, int64_t *bit_sweeps, int64_t *voxel_sweeps);
/* first retraces of an edge list launched since the context was created: by the lean kernel of one GPU (k_refine_trace_lean: a
 * whole-grid table of whole bricks with valid neighbour bits, the labels of the last neargrid assignment on a grid of at least
 * 16 voxels per axis, no vacuum, at most 2^27 voxels) and by the generic kernel (everything else, and everything under
 * XB_CHECK_GENERIC_RETRACE) */
int xb_retrace_stats(xb_ctx *c, int64_t *lean_launches, int64_t *generic_launches);
/* launches of the persistent group trace since the context was created, by the walker that ran: the lean walker on a packed
 * position with neighbour bits (one GPU: a whole-grid table of whole bricks that vouches for its neighbour bits), the lean walker
 * with the brick-label lookup (cut bricks, slabs, XB_CHECK_BRICK_LOOKUP), and the generic walker (index products beyond 24
 * bits, XB_CHECK_GENERIC_WALKER); and how many of the first two took 64-bit table offsets (a table window of more than 2^27
 * voxels; up to there a lean walker forms 32-bit byte offsets) */
int xb_trace_stats(xb_ctx *c, int64_t *nb_lean_launches, int64_t *lookup_lean_launches, int64_t *generic_launches,
                   int64_t *wide_lean_launches);
/* with XB_DBG_KEEP_RETRACE_OVERFLOW set: the start voxels those retraces have put on their overflow lists since the last call that
 * took them, in list order, launch after launch.  *n is set to their number; they are copied and forgotten when `capacity`
 * (ints) holds them all */
int xb_retrace_overflow(xb_ctx *c, int32_t *out, int64_t capacity, int64_t *n);
/* after xb_edge_find, while its edge list is valid (nothing has rewritten `known` since): the list as the sweep left it -- voxel
 * indices, tile by tile in the order the tiles' workgroups arrived, by row and z inside a tile -- and how many tiles the sweep
 * listed (-1: this edge_find swept without a tile list).  `capacity` in ints; *edges is set even where the list does not fit. */
int xb_edge_list(xb_ctx *c, int32_t *out, int64_t capacity, int64_t *edges, int64_t *tiles_listed);
/* region growth: assignments repeated because the scheduled kill launches (XB_OPT_KILL_LAUNCHES; 6 after a chase) did not reach the
 * fixpoint, and the schedule this context uses now (raised to the worst case by the first repeat) */
int xb_growth_stats(xb_ctx *c, int64_t *retries, int64_t *kill_launches);

/* ---- multi-GPU transport: RCCL over xGMI, one process per GPU (no PyTorch) ------------------------------------
 * Replaces nothing in the reference -- its thread blocks share one address space (thread_handlers.py:28-58,
 * 154-205); these calls move what the slab scheduler (pybader_amd/slab.py) has to move between GPUs.  librccl is
 * loaded on the first call.  Rank 0 makes the unique id, the host side distributes its 128 bytes. */
int xb_comm_unique_id(uint8_t id_out[128]);
int xb_comm_init(xb_ctx *c, int rank, int nranks, const uint8_t id_in[128]);
int xb_comm_destroy(xb_ctx *c);
/* planes [xa, xb) of the label (which 0) / known (which 1) array to and from ring neighbours, one ncclGroup */
int xb_comm_exchange_planes(xb_ctx *c, int which, int n_send, const int32_t *send_peer, const int64_t *send_xa,
                            const int64_t *send_xb, int n_recv, const int32_t *recv_peer, const int64_t *recv_xa,
                            const int64_t *recv_xb);
/* n int64 reduced in place over the ranks (op 0 sum, 1 min, 2 max): the counters thread_handlers.refine sums */
int xb_comm_allreduce_i64(xb_ctx *c, int64_t *inout, int64_t n, int op);
/* n int64 from every rank, out[size * n] in rank order: maxima tables (thread_handlers.py:59-65), seeds */
int xb_comm_allgather_i64(xb_ctx *c, const int64_t *in, int64_t n, int64_t *out);
/* every rank's chunk [first[r], first[r]+count[r]) of the brick move masks (xb_brick_masks) and of the bricks'
 * single-maximum voxels to every rank */
int xb_comm_share_brick_masks(xb_ctx *c, const int64_t *first, const int64_t *count);
/* blocks 0-4 of the device-driven slab step: part [first[r], first[r] + count[r]) (bytes) from rank r to every rank;
 * block 5: summed := sum over the ranks of local.  Ordered on the context's stream, no host wait. */
int xb_comm_allgather_block(xb_ctx *c, int which, const int64_t *first, const int64_t *count);
int xb_comm_allreduce_block(xb_ctx *c);
/* what the communicator says about the run: out = {ncclCommCount, ncclCommUserRank, ncclCommCuDevice, ncclGetVersion}
 * (-1 where this librccl lacks the entry point) -- lets a multi-GPU bench line prove it ran on N ranks and N devices */
int xb_comm_info(xb_ctx *c, int64_t out[4]);
/* plane bytes this rank has sent since xb_comm_init (label halos travel as dtype_calc(-n_maxima): int8 for up to 127 basins) */
int xb_comm_stats(xb_ctx *c, int64_t *bytes_sent);

#ifdef __cplusplus
}
#endif
#endif /* BADER_HIP_H */
