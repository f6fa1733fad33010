// host_analyses.h -- host side, part 20 (after every analysis): what the analyses give up together.  Their device blocks and the
// table of which a change of shape releases are ctx_buffers.h's; what each keeps of its last call on the host goes in its own
// *_forget.  An analysis that caches a result of the grid or keeps a block adds its line HERE and its row THERE, nowhere else.

// free_grid (shape_only false): every result and every block.  xb_set_grid on a change of the grid's shape (shape_only true): the
// results made for the old shape -- the Hirshfeld setup too, whose block stays to be refilled -- and the blocks the table names;
// the weight method's results and the per-call buffers of the other analyses belong to the voxel count and stay.
static void analyses_forget(xb_ctx *c, bool shape_only) {
    adjacency_forget(c); merge_forget(c); critical_forget(c); hirshfeld_forget(c); isosurface_forget(c); regions_forget(c);
    if (shape_only) { buf_release_on_shape_change(*c, HipMem{c->stream}); return; }
    c->w_have = false;
    buf_release_all(*c, HipMem{c->stream});
}

// the xb_*_release calls: after the work queued on the context's stream, the analysis forgets its results and gives the blocks
// first .. last back; the next call of the analysis allocates them again
static int analysis_release(xb_ctx *c, const char *who, void (*forget)(xb_ctx *), int first, int last) {
    if (!c) return fail(XB_E_ARG, "%s: null ctx", who);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    forget(c);
    release(c, first, last);
    return XB_OK;
}
int xb_weight_release(xb_ctx *c) { return analysis_release(c, "xb_weight_release", weight_forget, BLK_W_A, BLK_W_STATE); }
int xb_adjacency_release(xb_ctx *c) { return analysis_release(c, "xb_adjacency_release", adjacency_forget, BLK_AJ, BLK_AJ); }
int xb_merge_release(xb_ctx *c) { return analysis_release(c, "xb_merge_release", merge_forget, BLK_MG, BLK_MG); }
int xb_critical_release(xb_ctx *c) { return analysis_release(c, "xb_critical_release", critical_forget, BLK_CP_LIST, BLK_CP_LUT); }
int xb_hirshfeld_release(xb_ctx *c) { return analysis_release(c, "xb_hirshfeld_release", hirshfeld_forget, BLK_HS, BLK_HS); }
int xb_isosurface_release(xb_ctx *c) { return analysis_release(c, "xb_isosurface_release", isosurface_forget, BLK_ISO_VERT, BLK_ISO_WRAP); }
int xb_regions_release(xb_ctx *c) { return analysis_release(c, "xb_regions_release", regions_forget, BLK_RG_MAP, BLK_RG_SEED); }
