// ctx_state.h -- which derived state of a context (xb_ctx inherits CtxState) still matches the density and the labels on the
// card, and the events that drop it.  Plain C++, no include: tests/test_ctx_state_cpu.py compiles it alone and pins each function.
#pragma once
struct CtxState {
    bool has_vacuum = true;    // false only when volumes_init proved there is no -1 label
    bool vac_by_tol = false;   // the -1 labels are exactly the voxels with rho <= vac_tol (xb_vacuum_assign wrote them, nobody since)
    bool buni_valid = false;       // per-brick label uniformity (in `st`) matches the resident labels
    bool regions_labels = false;   // the resident labels are the last neargrid assignment's (+ refinement): every voxel of a
                                   // trapping-region brick (blab > 0) still carries the region's label
    bool grad_valid = false;
    bool grad_nb = false;      // every record of the resident table carries neighbour bits (bader_kernels.h) that match the bricks that hold
                               // records now: set by the pass-B launches that write a whole-grid table of whole bricks (launch_brick_records),
                               // cleared with grad_valid and by every other writer of records; nb_bits_ok() is what the launchers ask
    bool brick_max_valid = false;   // brick_rec bit 1 (the brick holds a 26-neighbour maximum) is right for the density on the card
    bool labels_zero_pending = false;   // volumes_init without vacuum: labels := 0 is owed (see xb_vacuum_assign)
    int zero_outside[3] = {-1, -1, -1}; // slab (x0, x1, halo) for which every label outside the planes [x0-halo, x1+halo) is known to be 0
    int label_wire = 4;        // bytes per label that hold EVERY resident label (1 / 2 / 4): what the narrowed halo may travel in.
                               // Follows whoever wrote the labels last: an assignment (dtype_calc(-n_maxima)), an upload (its dtype),
                               // volume_assign (the largest atom index) -- calls every rank of a slab run makes alike, so the
                               // ranks agree on it (send / receive sizes).  Planes or voxels written from outside widen it only
                               // if one of their labels does not fit; xb_label_wire lets a scheduler agree on the maximum
    int chg_n = -1;            // >= 0: the upper half of `stage` lists the chg_n voxels the last retrace pass relabelled (all known == -2 voxels)
    bool list_valid = false;   // the first list_n entries of `list` hold the owned known == -2 voxels (set by xb_edge_find)
    // the results of xb_critical_points, xb_isosurface, xb_regions_label are the resident density's (set by their owners)
    bool cp_have = false, iso_have = false, rg_have = false;
    // has anything been put into the density / the labels of this grid?  (xb_moment_sum refuses a grid without; set by every
    // call that writes them or hands their pointer out, cleared when the grid's shape changes)
    bool have_rho = false, have_labels = false;
};

// primitives: a group of stores that recurs
static inline void drop_table(CtxState &s) { s.grad_valid = false; s.grad_nb = false; }
static inline void drop_table_and_maxima(CtxState &s) { drop_table(s); s.brick_max_valid = false; }
// `stage` or `known` was rewritten: the upper half of `stage` may have listed the voxels the last retrace pass changed
static inline void stage_clobbered(CtxState &s) { s.chg_n = -1; }
static inline void drop_edge_lists(CtxState &s) { s.list_valid = false; stage_clobbered(s); }
static inline void drop_label_marks(CtxState &s) { s.buni_valid = false; s.regions_labels = false; }
// the one place where an analysis that caches a result of the density registers its flag
static inline void drop_density_results(CtxState &s) { s.cp_have = false; s.iso_have = false; s.rg_have = false; }
// the -1 labels no longer say "rho <= vac_tol" of the density on the card (raised before the grid check: a refused call drops it too)
static inline void vacuum_marks_unproven(CtxState &s) { s.vac_by_tol = false; }
// events.  Every voxel of the density is rewritten / its pointer is handed out: whoever holds it may write it (the table stays)
static inline void density_written(CtxState &s) { drop_table_and_maxima(s); s.have_rho = true; drop_density_results(s); }
static inline void density_pointer_out(CtxState &s) { s.have_rho = true; drop_density_results(s); }
// every label is overwritten from outside an assignment; `wire` bytes hold each new one
static inline void labels_overwritten(CtxState &s, int wire, bool has_vacuum) {
    s.labels_zero_pending = false; s.zero_outside[0] = -1; drop_edge_lists(s); drop_label_marks(s);
    s.has_vacuum = has_vacuum; s.vac_by_tol = false;
    s.label_wire = wire; s.have_labels = true;
}
// SOME labels are overwritten from outside an assignment (xb_scatter_voxels, label planes of xb_copy_planes, the results of
// xb_walkers_apply): the -1 labels are no longer xb_vacuum_assign's alone, and a negative label among the written ones brings the
// vacuum back.  `wire` bytes hold each written label: the resident width only grows (see label_wire).  `marks_kept`: which
// label marks the writer vouches for -- LABEL_MARKS_NONE; LABEL_MARKS_REGIONS: the written labels are retrace results or a
// slab's halo planes from peers that ran the same assignment, a region's brick keeps the region's label; LABEL_MARKS_BOTH:
// halo planes that the uniformity marks do not cover either.  `owned_only`: every written voxel lies in the owned planes (what
// zero_outside says of the others stays true)
enum { LABEL_MARKS_NONE = 0, LABEL_MARKS_REGIONS = 1, LABEL_MARKS_BOTH = 2 };
static inline void labels_patched(CtxState &s, int wire, bool any_negative, int marks_kept, bool owned_only) {
    vacuum_marks_unproven(s);
    if (any_negative) s.has_vacuum = true;
    drop_edge_lists(s); s.have_labels = true;
    if (!owned_only) s.zero_outside[0] = -1;
    if (wire > s.label_wire) s.label_wire = wire;
    if (marks_kept < LABEL_MARKS_BOTH) s.buni_valid = false;
    if (marks_kept < LABEL_MARKS_REGIONS) s.regions_labels = false;
}
