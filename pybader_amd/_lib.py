"""ctypes binding of libbader_hip.so (include/bader_hip.h).  No PyTorch, no CPU fallback: if the
library or a GPU is missing, every entry point raises."""
import ctypes as C
import threading
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('XB_LIBRARY') or os.path.join(HERE, 'libbader_hip.so')   # (XB_LIBRARY: A/B runs of two builds)

METHODS = {'ongrid': 0, 'neargrid': 1}          # methods.__contains__ (methods.py:12)
REFINE_MODES = {'all': 0, 'changed': 1}         # refine_mode[0] (thread_handlers.py:201-205)
DTYPE_CODE = {np.dtype(np.int8): 1, np.dtype(np.int16): 2, np.dtype(np.int32): 4, np.dtype(np.int64): 8}
# the int64 entries of the slab step's block 5 (the XB_XC_* enum of include/bader_hip.h)
(XB_XC_EDGES, XB_XC_CHANGED, XB_XC_ESCAPED, XB_XC_TRAVELLING, XB_XC_SLOW, XB_XC_LOST, XB_XC_MINE, XB_XC_ROUNDS,
 XB_XC_COUNT) = range(9)
# xb_kernel_time's `which` (the XB_TIMER_* enum; like every value below frozen: benchmarks pass them as plain integers)
(XB_TIMER_ASSIGN, XB_TIMER_OG_MASKS, XB_TIMER_EDGE_FIND, XB_TIMER_REFINE_TRACE, XB_TIMER_MASKS_GROWTH, XB_TIMER_BRICK_MASKS,
 XB_TIMER_TRACE, XB_TIMER_BRICK_RECORDS, XB_TIMER_MOMENTS, XB_TIMER_ADJACENCY, XB_TIMER_MERGE, XB_TIMER_COUNT) = range(12)
# xb_set_option's `key` (the XB_OPT_* enum), each key's value on the lines after it
XB_OPT_REGIONS = 1
XB_REGIONS_BOXES, XB_REGIONS_BRICKS = 1, 2
XB_OPT_CROSS_CHECK = 2
(XB_CHECK_NO_MIRROR, XB_CHECK_GENERIC_WALKER, XB_CHECK_FULL_TGRAD, XB_CHECK_LIST_DILATE, XB_CHECK_WIDE_HALO,
 XB_CHECK_NO_EC_SHARE, XB_CHECK_IO_GATHER) = (1, 2, 4, 8, 16, 32, 64)
CROSS_CHECK_BRICK_LOOKUP = 128   # the header's macro XB_CHECK_BRICK_LOOKUP, one more bit of XB_OPT_CROSS_CHECK (its enumerators are pinned)
CROSS_CHECK_VOXEL_SWEEP = 256    # XB_CHECK_VOXEL_SWEEP, likewise: the per-voxel edge sweep + the dilation kernel instead of row bit masks
CROSS_CHECK_GENERIC_RETRACE = 512   # XB_CHECK_GENERIC_RETRACE, likewise: the generic retrace kernel where the lean one would run
XB_OPT_DEBUG = 3
XB_DBG_EC_PASSES, XB_DBG_SLAB_STATS, XB_DBG_STAGE_WAIT, XB_DBG_SHORT_TIERS = 4, 16, 32, 64
DEBUG_KEEP_RETRACE_OVERFLOW = 128   # the header's macro XB_DBG_KEEP_RETRACE_OVERFLOW, one more bit of XB_OPT_DEBUG (its enumerators are pinned)
XB_OPT_EC_GROUPS = 4
XB_OPT_EC_QCAP = 5
XB_OPT_DROP_TABLE = 6
XB_DROP_TABLE_AND_MAXIMA = 2
XB_OPT_KILL_LAUNCHES = 17
XB_OPT_SELF_EXCHANGE = 19
XB_OPT_ASYNC_COMM = 24
XB_OPT_WEIGHT_NO_LABELS = 30
# xb_voronoi_assign: the bit of `flags` that makes every tile search all images, and the candidates a tile's list holds
XB_VORONOI_FULL_SEARCH = 1
XB_VORONOI_CAND_MAX = 512
# xb_critical_points: the bit of `flags` that counts components by flood fill instead of the table; the entries of counts[];
# the lower mask of a maximum and the size of xb_critical_lut's table
XB_CRITICAL_FLOOD = 1
(XB_CRITICAL_MAXIMA, XB_CRITICAL_BOND_VOXELS, XB_CRITICAL_BOND_SUM, XB_CRITICAL_RING_VOXELS, XB_CRITICAL_RING_SUM,
 XB_CRITICAL_MINIMA, XB_CRITICAL_COUNTS) = range(7)
XB_CRITICAL_FULL = 0x3fff
XB_CRITICAL_LUT_SIZE = 16384
# xb_laplacian_field / xb_laplacian_sum: the bit of `flags` that reads the 19 values from global memory instead of staging tiles;
# the doubles xb_stencil_coeffs writes and the doubles per voxel of xb_stencil_points
XB_STENCIL_GATHER = 1
XB_STENCIL_COEFFS = 51
XB_STENCIL_POINT_VALUES = 10
# xb_nci_field / xb_nci_sum / xb_nci_hist: C = 2 (3 pi^2)^(1/3) of the reduced gradient (the header's macro XB_NCI_C, the same
# double), the classes of the region, the bins up to which a block counts in LDS and the most bins a histogram may have
NCI_C = float.fromhex('0x1.8bfd4dd6882cbp+2')
XB_NCI_ATTRACTIVE, XB_NCI_VDW, XB_NCI_REPULSIVE, XB_NCI_CLASSES = range(4)
XB_NCI_HIST_LDS_BINS = 1024
XB_NCI_BINS_MAX = 1 << 24
# xb_isosurface: the bit of `flags` that reads the cube's corners from global memory instead of staging tiles; the bytes of
# xb_isosurface_table; what xb_isosurface_nci_mask raises s to (the header's macro XB_ISO_NCI_RAISED)
XB_ISO_GATHER = 1
XB_ISO_TABLE_SIZE = 768
ISO_NCI_RAISED = 100.0
# xb_regions_label: the modes, the bits of `flags` (the second route; the list route of xb_regions_shares; the NCI predicate's
# values from global memory) and the cell count up to which the shares use a dense table
XB_DOMAINS_ABOVE = 0
XB_DOMAINS_BELOW = 1
XB_DOMAINS_NCI = 2
XB_DOMAINS_GLOBAL = 1
XB_DOMAINS_SHARES_LIST = 2
XB_DOMAINS_GATHER = 4
XB_DOMAINS_TIMES = 8
XB_DOMAINS_SHARE_CELLS = 1 << 24
# xb_hirshfeld_sum / xb_hirshfeld_field: the bit of `flags` that makes every tile run over the whole image list, the candidates a
# tile's list holds, and the two modes of the field
XB_HIRSHFELD_FULL_SEARCH = 1
XB_HIRSHFELD_CAND_MAX = 256
XB_HIRSHFELD_PROMOLECULE, XB_HIRSHFELD_DEFORMATION = 0, 1
# xb_isa_iterate: the bit of `flags` (beside XB_HIRSHFELD_FULL_SEARCH) that sends every pair out with a global atomic of its own,
# and the most iterations one call queues
XB_ISA_DIRECT = 2
XB_ISA_ITERS_MAX = 64
# xb_mbis_iterate: XB_MBIS_DIRECT sends every pair and shell out with a global atomic of its own, XB_MBIS_KEEP (one iteration only)
# leaves the parameters as they are; at most XB_MBIS_SHELLS_MAX shells per atom
XB_MBIS_DIRECT = 2
XB_MBIS_KEEP = 4
XB_MBIS_ITERS_MAX = 64
XB_MBIS_SHELLS_MAX = 8
# xb_stockholder_moments: the bit of `flags` (beside XB_HIRSHFELD_FULL_SEARCH) that sends every pair and bin out with a global atomic
# of its own
XB_STOCKMOM_DIRECT = 2
# xb_igm_field: the modes (the atomic gradients are the free atoms' own, or the stockholder shares of the density's), the most fragments
XB_IGM_PRO, XB_IGM_STOCKHOLDER = 0, 1
XB_IGM_FRAGMENTS_MAX = 4

# every symbol include/bader_hip.h declares: (restype, argtypes)
_vp, _i64, _dbl, _int = C.c_void_p, C.c_int64, C.c_double, C.c_int
_pi64, _pdbl = C.POINTER(C.c_int64), C.POINTER(C.c_double)
SYMBOLS = {
    'xb_last_error': (C.c_char_p, []),
    'xb_device_count': (_int, []),
    'xb_create': (_int, [_int, C.POINTER(_vp)]),
    'xb_destroy': (None, [_vp]),
    'xb_sync': (_int, [_vp]),
    'xb_stream': (_vp, [_vp]),
    'xb_set_grid': (_int, [_vp, _pi64, _pdbl, _pdbl, _i64, _i64]),
    'xb_upload_density': (_int, [_vp, _vp]),
    'xb_synth_density': (_int, [_vp, _pdbl, _pdbl, _i64, _dbl]),
    'xb_parse_density_text': (_int, [_vp, _vp, _i64, _dbl, _pi64, _pi64]),
    'xb_parse_cube_text': (_int, [_vp, _vp, _i64, _i64, _i64, _int, _dbl, _pi64, _pi64]),
    'xb_download_density': (_int, [_vp, _vp]),
    'xb_format_begin': (_int, [_vp, _vp, _pi64, _int, _dbl, _int, _int, _vp, _i64, _i64, _pi64]),
    'xb_format_host_values': (_int, [_vp, _vp, _vp]),
    'xb_format_set_host_text': (_int, [_vp, _vp, _vp]),
    'xb_format_next': (_int, [_vp, C.POINTER(_vp), _pi64]),
    'xb_format_times': (_int, [_vp, _pdbl, _pdbl]),
    'xb_format_end': (_int, [_vp]),
    'xb_upload_labels': (_int, [_vp, _vp, _int]),
    'xb_download_labels': (_int, [_vp, _vp, _int]),
    'xb_import_density': (_int, [_vp, _vp, _int, _pi64, _vp]),
    'xb_import_labels': (_int, [_vp, _vp, _int, _vp]),
    'xb_export_labels': (_int, [_vp, _vp, _int, _vp]),
    'xb_export_volume': (_int, [_vp, _i64, _vp, _int, _vp]),
    'xb_device_alloc': (_int, [_int, _i64, C.POINTER(_vp)]),
    'xb_device_free': (_int, [_vp]),
    'xb_device_read': (_int, [_vp, _vp, _vp, _i64, _vp]),
    'xb_upload_known': (_int, [_vp, _vp]),
    'xb_download_known': (_int, [_vp, _vp]),
    'xb_vacuum_assign': (_int, [_vp, _dbl, _dbl, _pdbl, _pdbl]),
    'xb_assign': (_int, [_vp, _int, _pi64]),
    'xb_get_maxima': (_int, [_vp, _vp, _i64]),
    'xb_assign_trace': (_int, [_vp, _int, _pi64]),
    'xb_assign_local_table': (_int, [_vp, _vp, _vp, _i64]),
    'xb_assign_finish': (_int, [_vp, _vp, _i64]),
    'xb_prepare_refine': (_int, [_vp]),
    'xb_edge_find': (_int, [_vp, _pi64]),
    'xb_refine_trace': (_int, [_vp, _pi64, _pi64]),
    'xb_refine_trace_escaped': (_int, [_vp, _pi64, _pi64]),
    'xb_escaped_paths': (_int, [_vp, _i64, _pi64, _pi64]),
    'xb_escaped_paths_fetch': (_int, [_vp, _vp, _vp, _vp, _vp]),
    'xb_gather_voxels': (_int, [_vp, _vp, _i64, _vp, _vp]),
    'xb_scatter_voxels': (_int, [_vp, _vp, _i64, _vp, _vp]),
    'xb_walkers_count': (_int, [_vp, _pi64, _pi64]),
    'xb_walkers_fetch': (_int, [_vp, _vp, _vp]),
    'xb_walkers_continue': (_int, [_vp, _vp, _i64]),
    'xb_walkers_apply': (_int, [_vp, _vp, _i64, _pi64, _pi64]),
    'xb_edge_check': (_int, [_vp, _pi64, _pi64]),
    'xb_edge_check_local': (_int, [_vp, _pi64]),
    'xb_edge_check_local_fetch': (_int, [_vp, _vp, _vp]),
    'xb_edge_check_global': (_int, [_vp, _vp, _vp, _i64, _pi64, _pi64]),
    'xb_refine': (_int, [_vp, _int, _i64, _vp, _i64, _pi64]),
    'xb_assign_refine': (_int, [_vp, _int, _int, _i64, _pi64, _vp, _i64, _pi64]),
    'xb_charge_sum': (_int, [_vp, _dbl, _i64, _vp, _vp]),
    'xb_moment_sum': (_int, [_vp, _pdbl, _pdbl, _i64, _dbl, _pdbl, _pdbl]),
    'xb_adjacency': (_int, [_vp, _vp, _int, _i64, _pi64]),
    'xb_adjacency_fetch': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64]),
    'xb_adjacency_release': (_int, [_vp]),
    'xb_merge_basins': (_int, [_vp, _vp, _int, _i64, _vp, _dbl, _i64, _pi64, _pi64, C.POINTER(_int)]),
    'xb_merge_fetch': (_int, [_vp, _vp, _vp, _vp, _i64]),
    'xb_merge_release': (_int, [_vp]),
    'xb_weight_sum': (_int, [_vp, _pdbl, _dbl, _vp, _pi64]),
    'xb_weight_sum_device': (_int, [_vp, _pdbl, _dbl, _vp, _int, _pi64, _vp, _pi64]),
    'xb_weight_fetch': (_int, [_vp, _vp, _vp, _vp, _i64]),
    'xb_weight_stats': (_int, [_vp, _pi64]),
    'xb_weight_release': (_int, [_vp]),
    'xb_voronoi_assign': (_int, [_vp, _pdbl, _pdbl, _i64, _dbl, _int, _pi64]),
    'xb_critical_lut': (_int, [_vp]),
    'xb_critical_points': (_int, [_vp, _dbl, _int, _pi64, _pi64]),
    'xb_critical_fetch': (_int, [_vp, _vp, _vp, _vp, _vp, _i64]),
    'xb_critical_bonds': (_int, [_vp, _i64, _pi64, _pi64]),
    'xb_critical_bonds_fetch': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64]),
    'xb_critical_release': (_int, [_vp]),
    'xb_stencil_coeffs': (_int, [_pdbl, _i64, _i64, _i64, _pdbl]),
    'xb_laplacian_field': (_int, [_vp, _pdbl, _int, _vp, _vp]),
    'xb_laplacian_sum': (_int, [_vp, _pdbl, _i64, _dbl, _int, _pdbl, _pdbl, _pdbl]),
    'xb_stencil_points': (_int, [_vp, _pdbl, _vp, _i64, _vp]),
    'xb_nci_field': (_int, [_vp, _pdbl, _int, _vp, _vp, _vp, _vp]),
    'xb_nci_sum': (_int, [_vp, _pdbl, _i64, _dbl, _dbl, _dbl, _dbl, _int, _pi64, _pdbl, _pdbl]),
    'xb_nci_hist': (_int, [_vp, _pdbl, _pdbl, _i64, _pdbl, _i64, _int, _pi64]),
    'xb_dori_field': (_int, [_vp, _pdbl, _dbl, _int, _vp, _vp, _vp, _vp]),
    'xb_dori_sum': (_int, [_vp, _pdbl, _i64, _dbl, _dbl, _dbl, _dbl, _int, _pi64, _pdbl, _pdbl]),
    'xb_igm_field': (_int, [_vp, _pdbl, _vp, _int, _int, _dbl, _int, _vp, _vp, _vp, _vp, _pi64]),
    'xb_igm_sum': (_int, [_vp, _vp, _vp, _i64, _dbl, _dbl, _dbl, _pi64, _pdbl, _pdbl]),
    'xb_isosurface_table': (_int, [_vp]),
    'xb_isosurface': (_int, [_vp, _vp, _vp, _pdbl, _dbl, _i64, _int, _pi64]),
    'xb_isosurface_fetch': (_int, [_vp, _int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _pdbl, _pdbl, _i64]),
    'xb_isosurface_release': (_int, [_vp]),
    'xb_isosurface_nci_mask': (_int, [_vp, _vp, _dbl]),
    'xb_regions_label': (_int, [_vp, _int, _vp, _dbl, _pdbl, _dbl, _dbl, _int, _pi64]),
    'xb_regions_sums': (_int, [_vp, _dbl, _dbl, _pi64, _pi64, _pi64, _pdbl, _pdbl, _pi64, _pdbl, _pdbl, _i64]),
    'xb_regions_shares': (_int, [_vp, _i64, _int, _pi64]),
    'xb_regions_shares_fetch': (_int, [_vp, _vp, _vp, _pi64, _i64]),
    'xb_regions_fetch_map': (_int, [_vp, _int, _vp]),
    'xb_regions_times': (_int, [_vp, _pdbl]),
    'xb_regions_release': (_int, [_vp]),
    'xb_stream_wait': (_int, [_vp, _vp]),
    'xb_device_write': (_int, [_vp, _vp, _vp, _i64]),
    'xb_hirshfeld_images': (_int, [_pdbl, _pdbl, _vp, _i64, _pdbl, _i64, _pi64, _vp, _i64]),
    'xb_hirshfeld_setup': (_int, [_vp, _pdbl, _pdbl, _vp, _i64, _pdbl, _pdbl, _i64, _i64]),
    'xb_hirshfeld_release': (_int, [_vp]),
    'xb_hirshfeld_sum': (_int, [_vp, _dbl, _int, _pdbl, _pdbl, _pdbl, _pi64]),
    'xb_hirshfeld_field': (_int, [_vp, _int, _int, _vp, _vp]),
    'xb_isa_setup': (_int, [_vp, _pdbl, _pdbl, _i64, _pdbl, _i64, _pdbl, _dbl, _pi64]),
    'xb_isa_iterate': (_int, [_vp, _i64, _int, _pi64, _pi64]),
    'xb_isa_tables': (_int, [_vp, _pdbl, _pi64]),
    'xb_isa_load': (_int, [_vp, _pdbl]),
    'xb_isa_rho_bound': (_int, [_vp, _pdbl]),
    'xb_mbis_setup': (_int, [_vp, _pdbl, _pdbl, _i64, _pdbl, _vp, _pdbl, _i64, _i64, _pdbl, _pdbl, _dbl, _dbl, _pi64]),
    'xb_mbis_iterate': (_int, [_vp, _i64, _int, _pi64, _pi64, _pi64, _pi64]),
    'xb_mbis_params': (_int, [_vp, _pdbl, _pdbl, _pi64]),
    'xb_mbis_load': (_int, [_vp, _pdbl, _pdbl]),
    'xb_mbis_field': (_int, [_vp, _int, _int, _vp, _vp]),
    'xb_stockholder_moments': (_int, [_vp, _dbl, _int, _pi64, _pi64, _pi64]),
    'xb_volume_assign': (_int, [_vp, _vp, _i64]),
    'xb_atom_assign': (_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    'xb_surface_distance': (_int, [_vp, _vp, _vp, _i64, _vp, _pi64]),
    'xb_volume_mask': (_int, [_vp, _i64, _vp]),
    'xb_label_sum': (_int, [_vp, _i64, _pdbl, _pi64]),
    'xb_set_table_window': (_int, [_vp, _i64]),
    'xb_table_build': (_int, [_vp, _pi64]),
    'xb_table_local_seeds': (_int, [_vp, _vp, _i64]),
    'xb_brick_masks': (_int, [_vp, C.POINTER(_vp), _pi64, _pi64, _pi64]),
    'xb_table_ties': (_int, [_vp, _pi64]),
    'xb_table_finish': (_int, [_vp, _vp, _i64, _i64]),
    'xb_labels_ptr': (_vp, [_vp]),
    'xb_known_ptr': (_vp, [_vp]),
    'xb_density_ptr': (_vp, [_vp]),
    'xb_plane_elems': (_i64, [_vp]),
    'xb_copy_planes': (_int, [_vp, _int, _int, _vp, _i64, _i64]),
    'xb_label_wire': (_int, [_vp, _int, _vp]),
    'xb_host_alloc': (_int, [_i64, _vp]),
    'xb_host_free': (_int, [_vp]),
    'xb_brick_masks_copy': (_int, [_vp, _int, _vp, _i64, _i64]),
    'xb_set_halo': (_int, [_vp, _i64]),
    'xb_kernel_time': (_int, [_vp, _int, _pdbl, _pi64]),
    'xb_kernel_time_reset': (_int, [_vp]),
    'xb_enable_timing': (_int, [_vp, _int]),
    'xb_set_option': (_int, [_vp, _int, _int]),
    'xb_box_stats': (_int, [_vp, _pi64, _pi64]),
    'xb_brick_labels': (_int, [_vp, _vp, _i64, _pi64]),
    'xb_slow_path_stats': (_int, [_vp, _pi64, _pi64]),
    'xb_deferred_stats': (_int, [_vp, _pi64]),
    'xb_sweep_stats': (_int, [_vp, _pi64, _pi64]),
    'xb_edge_list': (_int, [_vp, _vp, _i64, _pi64, _pi64]),
    'xb_retrace_stats': (_int, [_vp, _pi64, _pi64]),
    'xb_trace_stats': (_int, [_vp, _pi64, _pi64, _pi64, _pi64]),
    'xb_axis_limits': (_int, [_vp, _pi64, _pi64]),
    'xb_retrace_overflow': (_int, [_vp, _vp, _i64, _pi64]),
    'xb_growth_stats': (_int, [_vp, _pi64, _pi64]),
    'xb_comm_unique_id': (_int, [_vp]),
    'xb_comm_init': (_int, [_vp, _int, _int, _vp]),
    'xb_comm_destroy': (_int, [_vp]),
    'xb_comm_exchange_planes': (_int, [_vp, _int, _int, _vp, _pi64, _pi64, _int, _vp, _pi64, _pi64]),
    'xb_comm_allreduce_i64': (_int, [_vp, _pi64, C.c_int64, _int]),
    'xb_comm_allgather_i64': (_int, [_vp, _pi64, C.c_int64, _pi64]),
    'xb_comm_share_brick_masks': (_int, [_vp, _pi64, _pi64]),
    'xb_comm_allgather_block': (_int, [_vp, _int, _pi64, _pi64]),
    'xb_comm_allreduce_block': (_int, [_vp]),
    'xb_slab_supported': (_int, [_vp, _int, _pi64]),
    'xb_slab_assign_masks': (_int, [_vp, _int, _int]),
    'xb_slab_assign_trace': (_int, [_vp]),
    'xb_slab_assign_finish': (_int, [_vp, _pi64, _pi64]),
    'xb_slab_refine_pass': (_int, [_vp]),
    'xb_slab_walkers_round': (_int, [_vp, _int, _int]),
    'xb_slab_walk_layout': (_int, [_vp, _pi64]),
    'xb_slab_walk_send': (_int, [_vp, _i64]),
    'xb_slab_refine_counts': (_int, [_vp, _pi64, _pi64]),
    'xb_slab_block': (_int, [_vp, _int, C.POINTER(_vp), _pi64, _pi64, _pi64]),
    'xb_slab_block_copy': (_int, [_vp, _int, _int, _vp, _i64, _i64]),
    'xb_host_waits': (_int, [_pi64]),
    'xb_comm_stats': (_int, [_vp, _pi64]),
    'xb_comm_info': (_int, [_vp, _pi64]),
    'xb_memory_stats': (_int, [_vp, _pi64, _pi64, _pi64]),
}

_lib = None


class BaderHipError(RuntimeError):
    """carries the library's XB_E_* code in `.code` (None for host-side failures)"""
    code = None


XB_E_ARG = -1     # a bad argument, or a number in the text that does not convert
XB_E_STATE = -3   # a call the context's state does not allow (no grid, a slab where the whole grid is needed)
XB_E_LIMIT = -4   # a size beyond what the library indexes
XB_E_SHORT = -6   # xb_parse_density_text / xb_parse_cube_text: the text holds fewer numbers than the grid needs


def load():
    """dlopen libbader_hip.so and bind every declared symbol; raises if the library is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BaderHipError(f"{LIB_PATH} is missing: build it with `python -m pybader_amd.build` "
                                "(hipcc, gfx950); pybader_amd has no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)      # AttributeError here == ABI drift; fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


# ---- result arrays in page-locked memory ----------------------------------------------------------------------------------
# bader_calc returns a NEW narrowed label array per call (thread_handlers.py:70-74).  As a plain numpy allocation that is fresh
# pageable memory every time: the device-to-host copy is staged through a pinned chunk, copied again and takes a page fault per
# 4 KiB (2 ms per call for 16 MB at 256^3 against 0.35 ms on the bus).  pinned_empty() hands out arrays that live in page-locked
# buffers from a small pool; a buffer returns to the pool when the last reference to its array is gone (weakref.finalize), so a
# loop of calls stops allocating after its first pass.  The arrays are ordinary ndarrays (picklable, writeable).
_POOL_KEEP = 4            # free buffers kept per size; more are given back to the driver
_POOL_MAX_BYTES = 4 << 30  # free page-locked bytes the pool may hold in total (a batch of CHGCARs of many shapes must not pin the host)


class _PinnedBuf:
    __slots__ = ('ptr', 'nbytes', '__weakref__')

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes

    @property
    def __array_interface__(self):
        return {'shape': (self.nbytes,), 'typestr': '|u1', 'data': (self.ptr, False), 'version': 3}


_pool = {}                 # nbytes -> free pointers of that size (insertion order of the sizes = age)
_pool_bytes = 0            # bytes of all free buffers
_pool_lock = threading.Lock()


def _host_free(ptr):
    if _lib is not None:
        _lib.xb_host_free(C.c_void_p(ptr))


def _pool_evict(need):
    """(lock held) give free buffers back to the driver, oldest size first, until `need` more bytes fit under the cap"""
    global _pool_bytes
    for size in list(_pool):
        free = _pool[size]
        while free and _pool_bytes + need > _POOL_MAX_BYTES:
            _host_free(free.pop())
            _pool_bytes -= size
        if not free:
            del _pool[size]
        if _pool_bytes + need <= _POOL_MAX_BYTES:
            return


def _pool_release(ptr, nbytes):
    global _pool_bytes
    with _pool_lock:
        free = _pool.get(nbytes)
        if nbytes > _POOL_MAX_BYTES or (free is not None and len(free) >= _POOL_KEEP):
            _host_free(ptr)
            return
        _pool_evict(nbytes)
        _pool.setdefault(nbytes, []).append(ptr)
        _pool_bytes += nbytes


def pinned_empty(shape, dtype):
    """np.empty(shape, dtype) in page-locked memory from the pool (np.empty for small arrays, and when the driver has no more
    page-locked memory to give: a pageable result is slower, not wrong)"""
    import weakref
    global _pool_bytes
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dtype.itemsize
    if nbytes < (1 << 20):
        return np.empty(shape, dtype)
    ptr = None
    with _pool_lock:
        free = _pool.get(nbytes)
        if free:
            ptr = free.pop()
            _pool_bytes -= nbytes
            if not free:
                del _pool[nbytes]
    if ptr is None:
        p = C.c_void_p()
        rc = load().xb_host_alloc(nbytes, C.byref(p))
        if rc != 0 or not p.value:
            with _pool_lock:          # make room once (every free buffer of another size) and try again
                _pool_evict(_POOL_MAX_BYTES)
            rc = load().xb_host_alloc(nbytes, C.byref(p))
            if rc != 0 or not p.value:
                return np.empty(shape, dtype)
        ptr = p.value
    buf = _PinnedBuf(ptr, nbytes)
    weakref.finalize(buf, _pool_release, ptr, nbytes)
    return np.asarray(buf).view(dtype).reshape(shape)      # (a view of the buffer's uint8 array, which keeps `buf` alive through .base)


def pool_owned(a):
    """`a` came from pinned_empty: its base is the buffer's own uint8 array, which nobody else holds"""
    return isinstance(a.base, np.ndarray) and isinstance(a.base.base, _PinnedBuf)


def _numpy_owned(a):
    """the memory of `a` was allocated by numpy itself (malloc / calloc: private anonymous pages) -- not a memmap, a shared-memory
    segment or any other foreign buffer, whose untouched pages are NOT zeros"""
    owner = a
    while isinstance(owner, np.ndarray) and owner.base is not None:
        if isinstance(owner, np.memmap):
            return False
        owner = owner.base
    return isinstance(owner, np.ndarray) and not isinstance(owner, np.memmap) and owner.flags.owndata


def fast_any(a):
    """np.any(a) for a C-contiguous array WITHOUT touching pages nobody has touched: a fresh np.zeros() array is untouched
    anonymous memory -- the kernel's pagemap says so per page (neither present nor swapped: it reads as zeros) -- and scanning
    it would fault every page in (4.7 ms for the 64 MB label array of a 256^3 grid, of a 5 ms call pair).  Pages that are in
    use are scanned.  Only for memory numpy allocated itself: in a file-backed or shared mapping (np.memmap, shared_memory) a
    page this process has not touched holds data all the same.  Anything else, or anything unexpected, is np.any."""
    import mmap
    n = a.nbytes
    if n < (1 << 22) or not a.flags.c_contiguous or not _numpy_owned(a):
        return bool(np.any(a))
    try:
        addr = a.ctypes.data
        ps = mmap.PAGESIZE
        first = -(-addr // ps)            # first whole page
        last = (addr + n) // ps           # one past the last whole page
        if last <= first:
            return bool(np.any(a))
        with open('/proc/self/pagemap', 'rb', buffering=0) as f:
            f.seek(first * 8)
            flags = np.frombuffer(f.read((last - first) * 8), np.uint64)
        if flags.size != last - first:
            return bool(np.any(a))
        if np.any((flags >> np.uint64(61)) & np.uint64(1)):      # bit 61: file-mapped or shared-anonymous page -- not ours to guess about
            return bool(np.any(a))
        used = (flags >> np.uint64(62)) != 0          # bit 63 present, bit 62 swapped
        b = a.reshape(-1).view(np.uint8)
        head, tail = first * ps - addr, (addr + n) - last * ps
        if (head and b[:head].any()) or (tail and b[n - tail:].any()):
            return True
        idx = np.flatnonzero(used)
        if idx.size == 0:
            return False
        if idx.size * 4 > flags.size:
            return bool(np.any(a))
        brk = np.flatnonzero(np.diff(idx) != 1)
        starts = np.concatenate(([idx[0]], idx[brk + 1]))
        ends = np.concatenate((idx[brk], [idx[-1]])) + 1
        return any(b[head + s * ps: head + e * ps].any() for s, e in zip(starts, ends))
    except (OSError, ValueError):
        return bool(np.any(a))


def check(rc):
    if rc != 0:
        err = BaderHipError(f"libbader_hip error {rc}: {load().xb_last_error().decode()}")
        err.code = rc
        raise err


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Context:
    """One GPU context: device-resident density / labels / known + the hot-path calls."""

    def __init__(self, device=0):
        self.lib = load()
        n = self.lib.xb_device_count()
        if n <= 0:
            raise BaderHipError("no HIP device visible: the MI355X path cannot run (no CPU fallback)")
        h = C.c_void_p()
        check(self.lib.xb_create(int(device), C.byref(h)))
        self.h = h
        self.device = int(device)
        self.shape = None
        # utils.resident(): identity of the host array the caller pinned / of the one whose content is on the device
        self.pinned_density = None
        self.resident_density = None
        # utils.track_labels(): identity of the host array whose content equals the device labels (inside resident() only)
        self.resident_labels = None
        self._labels_host = None
        self.n_maxima = 0
        self.hirshfeld_key = None   # hirshfeld._setup(): what the library's Hirshfeld setup was made from
        self._hirshfeld_atoms = 0

    def drop_label_token(self):
        """the device labels are about to change (or be replaced): no host array equals them any more"""
        a = getattr(self, '_labels_host', None)
        if a is not None and getattr(self, '_labels_was_writeable', False):
            a.flags.writeable = True
        self._labels_host = None
        self.resident_labels = None

    def close(self):
        if getattr(self, 'h', None):
            self.lib.xb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- residency --------------------------------------------------------------------------
    def set_grid(self, shape, dist_mat, T_grad, x_range=None):
        shape = tuple(int(s) for s in shape)
        if shape != getattr(self, 'shape', None):
            self.drop_label_token()     # (another grid: no host array equals the device labels any more)
            self.hirshfeld_key = None   # (nor does the library keep a Hirshfeld setup over a change of shape)
            self.resident_density = None    # (nor is any array's content the device density: xb_set_grid drops it with the shape)
        x0, x1 = (0, shape[0]) if x_range is None else x_range
        sh = np.array(shape, dtype=np.int64)
        dm, tg = _f64(dist_mat).reshape(27), _f64(T_grad).reshape(9)
        check(self.lib.xb_set_grid(self.h, sh.ctypes.data_as(_pi64), dm.ctypes.data_as(_pdbl),
                                   tg.ctypes.data_as(_pdbl), int(x0), int(x1)))
        self.shape = shape
        self.x_range = (int(x0), int(x1))

    def set_halo(self, halo):
        check(self.lib.xb_set_halo(self.h, int(halo)))

    def upload_density(self, rho):
        rho = _f64(rho)
        assert rho.shape == self.shape, (rho.shape, self.shape)
        self.resident_density = None
        check(self.lib.xb_upload_density(self.h, _ptr(rho)))

    def synth_density(self, lattice, atoms, background):
        lat, at = _f64(lattice).reshape(9), _f64(atoms)
        self.resident_density = None
        check(self.lib.xb_synth_density(self.h, lat.ctypes.data_as(_pdbl), at.ctypes.data_as(_pdbl),
                                        at.shape[0], float(background)))

    def download_density(self):
        out = np.empty(self.shape, dtype=np.float64)
        check(self.lib.xb_download_density(self.h, _ptr(out)))
        return out

    def upload_labels(self, labels):
        self.drop_label_token()
        labels = np.ascontiguousarray(labels)
        assert labels.shape == self.shape
        check(self.lib.xb_upload_labels(self.h, _ptr(labels), DTYPE_CODE[labels.dtype]))

    def download_labels(self, dtype=np.int32, out=None, pooled=False):
        if out is None:
            out = pinned_empty(self.shape, dtype) if pooled else np.empty(self.shape, dtype=dtype)
        assert out.flags.c_contiguous and out.shape == self.shape
        check(self.lib.xb_download_labels(self.h, _ptr(out), DTYPE_CODE[out.dtype]))
        return out

    # -- arrays that already live on the device (pybader_amd/device.py) ------------------------------
    def _refuse_shape(self, what, shape):
        err = BaderHipError(f'{what}: the device array has shape {tuple(shape)}, the grid {self.shape}')
        err.code = XB_E_ARG
        raise err

    def import_density(self, obj):
        """a float32 / float64 device array of any strides becomes the resident density (xb_import_density)"""
        from . import device
        d = device.describe(obj)
        if d.shape != self.shape:
            self._refuse_shape('import_density', d.shape)
        if d.dtype not in device.FLOAT_CODE:
            err = BaderHipError(f'import_density: dtype {d.dtype.name} is neither float32 nor float64')
            err.code = XB_E_ARG
            raise err
        self.resident_density = None
        st = (C.c_int64 * 3)(*d.strides)
        check(self.lib.xb_import_density(self.h, C.c_void_p(d.ptr), device.FLOAT_CODE[d.dtype], st, device.stream_for(d)))

    def _flat(self, what, obj, codes, writable):
        from . import device
        d = device.describe(obj, writable=writable)
        if d.shape != self.shape:
            self._refuse_shape(what, d.shape)
        if d.dtype not in codes or not d.c_contiguous:
            err = BaderHipError(f'{what}: a C-contiguous device array of {" / ".join(t.name for t in codes)} is required '
                                f'(got {d.dtype.name}, element strides {d.strides})')
            err.code = XB_E_ARG
            raise err
        return d, device.stream_for(d)

    def import_labels(self, obj):
        """a C-contiguous integer device array becomes the resident label map (xb_import_labels)"""
        d, stream = self._flat('import_labels', obj, DTYPE_CODE, False)
        self.drop_label_token()
        check(self.lib.xb_import_labels(self.h, C.c_void_p(d.ptr), DTYPE_CODE[d.dtype], stream))

    def export_labels(self, dtype=np.int32, out=None):
        """the resident label map into `out` (a writable C-contiguous integer device array), else into a new
        device.DeviceArray of `dtype`; returns it"""
        from . import device
        if out is None:
            out = device.DeviceArray(self, self.shape, dtype)
        d, stream = self._flat('export_labels', out, DTYPE_CODE, True)
        check(self.lib.xb_export_labels(self.h, C.c_void_p(d.ptr), DTYPE_CODE[d.dtype], stream))
        return out

    def export_volume(self, vol_num, dtype=np.float64, out=None):
        """utils.volume_mask on the device: the resident density where the label equals vol_num, zero elsewhere, into
        `out` (writable, C-contiguous, float32 / float64) or a new device.DeviceArray of `dtype`; returns it"""
        from . import device
        if out is None:
            out = device.DeviceArray(self, self.shape, dtype)
        d, stream = self._flat('export_volume', out, device.FLOAT_CODE, True)
        check(self.lib.xb_export_volume(self.h, int(vol_num), C.c_void_p(d.ptr), device.FLOAT_CODE[d.dtype], stream))
        return out

    def upload_known(self, known):
        known = np.ascontiguousarray(known, dtype=np.int8)
        check(self.lib.xb_upload_known(self.h, _ptr(known)))

    def download_known(self):
        out = np.empty(self.shape, dtype=np.int8)
        check(self.lib.xb_download_known(self.h, _ptr(out)))
        return out

    # -- hot path ---------------------------------------------------------------------------
    def vacuum_assign(self, vac_tol, voxel_volume):
        self.drop_label_token()
        a, b = C.c_double(), C.c_double()
        tol = float('nan') if vac_tol is None else float(vac_tol)
        check(self.lib.xb_vacuum_assign(self.h, tol, float(voxel_volume), C.byref(a), C.byref(b)))
        return a.value, b.value

    def assign(self, method):
        self.drop_label_token()
        n = C.c_int64()
        check(self.lib.xb_assign(self.h, METHODS[method], C.byref(n)))
        self.n_maxima = n.value
        return n.value

    def maxima(self):
        out = np.zeros((self.n_maxima, 3), dtype=np.int64)
        check(self.lib.xb_get_maxima(self.h, _ptr(out), self.n_maxima))
        return out

    def assign_trace(self, method):
        self.drop_label_token()
        n = C.c_int64()
        check(self.lib.xb_assign_trace(self.h, METHODS[method], C.byref(n)))
        m, f = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64)
        check(self.lib.xb_assign_local_table(self.h, _ptr(m), _ptr(f), n.value))
        return m, f

    def assign_finish(self, max_sorted):
        self.drop_label_token()
        ms = np.ascontiguousarray(max_sorted, dtype=np.int64)
        check(self.lib.xb_assign_finish(self.h, _ptr(ms), ms.shape[0]))
        self.n_maxima = int(ms.shape[0])

    def prepare_refine(self):
        check(self.lib.xb_prepare_refine(self.h))

    def edge_find(self):
        n = C.c_int64()
        check(self.lib.xb_edge_find(self.h, C.byref(n)))
        return n.value

    def refine_trace(self):
        self.drop_label_token()
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_refine_trace(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def refine_trace_escaped(self):
        self.drop_label_token()
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_refine_trace_escaped(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def parse_density_text(self, text, divisor):
        """the density block of a CHGCAR (bytes or a uint8 array, Fortran order) -> resident density / divisor;
        returns (numbers found, numbers converted by the host fallback)"""
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else text
        assert buf.dtype == np.uint8 and buf.flags.c_contiguous
        a, b = C.c_int64(), C.c_int64()
        self.resident_density = None            # also when the parse fails midway: rho is partly rewritten
        check(self.lib.xb_parse_density_text(self.h, _ptr(buf), buf.size, float(divisor), C.byref(a), C.byref(b)))
        return a.value, b.value

    def parse_cube_text(self, text, scale, nval=1, pick=0, accumulate=False):
        """the density block of a cube file (bytes or a uint8 array, C order, `nval` values per voxel) -> resident
        density: value `pick` of every voxel times `scale`, or (resident + value) * scale with `accumulate`;
        returns (numbers found, numbers converted by the host fallback)"""
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else text
        assert buf.dtype == np.uint8 and buf.flags.c_contiguous
        a, b = C.c_int64(), C.c_int64()
        self.resident_density = None            # also when the parse fails midway: rho is partly rewritten
        check(self.lib.xb_parse_cube_text(self.h, _ptr(buf), buf.size, int(nval), int(pick), int(bool(accumulate)),
                                          float(scale), C.byref(a), C.byref(b)))
        return a.value, b.value

    def format_density_text(self, values, scale, style, prec, layout):
        """The text of a density block as the reference's writers produce it (utils.python_format / fortran_format,
        io/vasp.py write, io/cube.py write), formatted on the device: `values` [x][y][z] float64 times `scale`, style
        'E' | 'E_space' | 'F', `prec` digits, layout 'chgcar' | 'cube'.  A generator of (chunk, n_host): `chunk` is a
        memoryview of whole lines valid until the next step, n_host the number of values the host formatted.  The
        resident density and labels are not touched."""
        from . import textfmt
        a = _f64(values)
        if a.ndim != 3:
            raise ValueError('format_density_text: a 3-d array is required')
        shape = np.array(a.shape, dtype=np.int64)
        p10 = textfmt.pow10_table()
        nh = C.c_int64()
        check(self.lib.xb_format_begin(self.h, _ptr(a), shape.ctypes.data_as(_pi64), textfmt.LAYOUTS[layout], float(scale),
                                       textfmt.STYLES[style], int(prec), _ptr(p10), textfmt.POW10_LO, textfmt.POW10_N,
                                       C.byref(nh)))
        try:
            n_host = nh.value
            idx = np.zeros(n_host, np.int64)
            vals = np.zeros(n_host, np.float64)
            check(self.lib.xb_format_host_values(self.h, _ptr(idx), _ptr(vals)))
            strings = textfmt.host_strings(vals, style, prec, p10) if n_host else []
            text = ''.join(strings).encode('ascii')
            off = np.zeros(n_host + 1, np.int64)
            off[1:] = np.cumsum([len(t) for t in strings], dtype=np.int64)
            buf = np.frombuffer(text + b'\0', dtype=np.uint8)
            check(self.lib.xb_format_set_host_text(self.h, _ptr(off), _ptr(buf)))
            self.format_host = (idx, vals)
            ptr, nb = C.c_void_p(), C.c_int64()
            while True:
                check(self.lib.xb_format_next(self.h, C.byref(ptr), C.byref(nb)))
                if nb.value == 0:
                    break
                yield memoryview((C.c_char * nb.value).from_address(ptr.value)).cast('B'), n_host
            fm, cm = C.c_double(), C.c_double()
            check(self.lib.xb_format_times(self.h, C.byref(fm), C.byref(cm)))
            self.format_times = (fm.value, cm.value)
        finally:
            self.lib.xb_format_end(self.h)

    def escaped_paths(self, max_len=1 << 15):
        """(starts, offsets, voxels, complete): for every parked (known == -6) voxel of the owned slab its start
        voxel followed by its trajectory from the first voxel outside the valid planes on; trajectories are
        followed for at most max_len voxels, complete[i] tells whether path i reached its maximum"""
        n, m = C.c_int64(), C.c_int64()
        check(self.lib.xb_escaped_paths(self.h, int(max_len), C.byref(n), C.byref(m)))
        starts = np.zeros(n.value, np.int64)
        offsets = np.zeros(n.value + 1, np.int64)
        vox = np.zeros(m.value, np.int64)
        complete = np.zeros(n.value, np.int8)
        check(self.lib.xb_escaped_paths_fetch(self.h, _ptr(starts), _ptr(offsets), _ptr(vox), _ptr(complete)))
        return starts, offsets, vox, complete.astype(bool)

    def gather_voxels(self, idx):
        idx = np.ascontiguousarray(idx, np.int64)
        lab = np.zeros(idx.size, np.int32)
        kn = np.zeros(idx.size, np.int8)
        check(self.lib.xb_gather_voxels(self.h, _ptr(idx), idx.size, _ptr(lab), _ptr(kn)))
        return lab, kn

    def scatter_voxels(self, idx, labels, known):
        self.drop_label_token()
        idx = np.ascontiguousarray(idx, np.int64)
        lab = np.ascontiguousarray(labels, np.int32)
        kn = np.ascontiguousarray(known, np.int8)
        check(self.lib.xb_scatter_voxels(self.h, _ptr(idx), idx.size, _ptr(lab), _ptr(kn)))

    def label_wire(self, widen_to=0):
        """bytes per label of a label halo on the wire; `widen_to` raises it (the ranks of a slab run must agree)"""
        w = C.c_int()
        check(self.lib.xb_label_wire(self.h, int(widen_to), C.byref(w)))
        return w.value

    WALKER_WORDS = 10

    def walkers(self):
        """(walkers, results) left by the last refine_trace / walkers_continue: (n, 10) int64 records of the retraces
        that left this rank's valid planes, and the (start voxel | label << 32) pairs of the ones it finished"""
        n, m = C.c_int64(), C.c_int64()
        check(self.lib.xb_walkers_count(self.h, C.byref(n), C.byref(m)))
        w = np.zeros((n.value, self.WALKER_WORDS), np.int64)
        r = np.zeros(m.value, np.int64)
        check(self.lib.xb_walkers_fetch(self.h, _ptr(w), _ptr(r)))
        return w, r

    def walkers_continue(self, walkers):
        w = np.ascontiguousarray(walkers, np.int64).reshape(-1, self.WALKER_WORDS)
        check(self.lib.xb_walkers_continue(self.h, _ptr(w), w.shape[0]))
        return self.walkers()

    def walkers_apply(self, results):
        """-> (changed, stuck)"""
        self.drop_label_token()
        r = np.ascontiguousarray(results, np.int64).reshape(-1)
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_walkers_apply(self.h, _ptr(r), r.size, C.byref(a), C.byref(b)))
        return a.value, b.value

    def edge_check(self):
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_edge_check(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def edge_check_local(self):
        """slabs: the owned changed voxels (int64 linear indices) and their edge&maximum class (int8)"""
        n = C.c_int64()
        check(self.lib.xb_edge_check_local(self.h, C.byref(n)))
        idx, cls = np.empty(n.value, np.int64), np.empty(n.value, np.int8)
        if n.value:
            check(self.lib.xb_edge_check_local_fetch(self.h, _ptr(idx), _ptr(cls)))
        return idx, cls

    def edge_check_global(self, idx, cls):
        """slabs: resolve the all-gathered list; returns (checked, new edges in the owned planes)"""
        idx, cls = np.ascontiguousarray(idx, np.int64), np.ascontiguousarray(cls, np.int8)
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_edge_check_global(self.h, _ptr(idx), _ptr(cls), idx.size, C.byref(a), C.byref(b)))
        return a.value, b.value

    def assign_refine(self, method, mode, iters):
        """bader_calc + refine in one library call (one host wait for both on the fused one-GPU neargrid path); -> (n_maxima, log)"""
        self.drop_label_token()
        cap = 4096
        log = np.zeros(cap, dtype=np.int64)
        n, k = C.c_int64(), C.c_int64()
        check(self.lib.xb_assign_refine(self.h, METHODS[method], REFINE_MODES[mode.lower()], int(iters), C.byref(n), _ptr(log), cap, C.byref(k)))
        m = min(k.value, cap // 2)
        self.n_maxima = n.value
        return n.value, [(int(log[2 * i]), int(log[2 * i + 1])) for i in range(m)]

    def refine(self, mode, iters):
        self.drop_label_token()
        cap = 4096
        log = np.zeros(cap, dtype=np.int64)
        n = C.c_int64()
        check(self.lib.xb_refine(self.h, REFINE_MODES[mode.lower()], int(iters), _ptr(log), cap, C.byref(n)))
        k = min(n.value, cap // 2)
        return [(int(log[2 * i]), int(log[2 * i + 1])) for i in range(k)]

    def charge_sum(self, voxel_volume, n_labels):
        ch, vo = np.zeros(n_labels, np.float64), np.zeros(n_labels, np.float64)
        check(self.lib.xb_charge_sum(self.h, float(voxel_volume), int(n_labels), _ptr(ch), _ptr(vo)))
        return ch, vo

    def moment_sum(self, lattice, centres, voxel_volume):
        """moments of the resident density per resident label about `centres` (Cartesian, [n, 3]; the cell's `lattice` a row per
        axis) over the owned planes (xb_moment_sum) -> (moments f64[n, 10]: m0, m1 x y z, m2 xx xy xz yy yz zz; volume f64[n])"""
        lat, ce = _f64(lattice).reshape(9), _f64(centres).reshape(-1, 3)
        n = ce.shape[0]
        mo, vo = np.zeros((n, 10), np.float64), np.zeros(n, np.float64)
        check(self.lib.xb_moment_sum(self.h, lat.ctypes.data_as(_pdbl), ce.ctypes.data_as(_pdbl), n, float(voxel_volume),
                                     mo.ctypes.data_as(_pdbl), vo.ctypes.data_as(_pdbl)))
        return mo, vo

    def adjacency(self, dirs, n):
        """which of the resident labels 0 .. n - 1 share a surface (xb_adjacency; `dirs` int[K, 3], the active directions) ->
        (pairs int32[P, 2] ascending with a < b, facets int64[P, K], saddle f64[P], saddle_facet int64[P])"""
        d = np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 3)
        k, np_ = d.shape[0], C.c_int64()
        check(self.lib.xb_adjacency(self.h, _ptr(d), k, int(n), C.byref(np_)))
        p = int(np_.value)
        a, b = np.zeros(p, np.int32), np.zeros(p, np.int32)
        facets, saddle, sfacet = np.zeros((p, k), np.int64), np.zeros(p, np.float64), np.zeros(p, np.int64)
        check(self.lib.xb_adjacency_fetch(self.h, _ptr(a), _ptr(b), _ptr(facets), _ptr(saddle), _ptr(sfacet), p))
        return np.stack([a, b], axis=1), facets, saddle, sfacet

    def adjacency_release(self):
        """free the pair table of xb_adjacency (it is kept between calls while the grid's shape stays) and the fetched pairs"""
        check(self.lib.xb_adjacency_release(self.h))

    def merge_basins(self, dirs, max_idx, tol, max_rounds=64):
        """merge the resident labels 0 .. n - 1 whose persistence lies below `tol`, round by round (xb_merge_basins; `dirs`
        int[K, 3], the active directions; `max_idx` int[n], the linear voxel of each label's maximum) ->
        (root int32[n], merge_round int32[n], merge_persistence f64[n], rounds, n_survivors, converged)"""
        d = np.ascontiguousarray(dirs, dtype=np.int32).reshape(-1, 3)
        idx = np.ascontiguousarray(max_idx, dtype=np.int64).reshape(-1)
        n, rounds, left, conv = idx.shape[0], C.c_int64(), C.c_int64(), C.c_int()
        check(self.lib.xb_merge_basins(self.h, _ptr(d), d.shape[0], n, _ptr(idx), float(tol), int(max_rounds), C.byref(rounds),
                                       C.byref(left), C.byref(conv)))
        root, rnd, pers = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
        check(self.lib.xb_merge_fetch(self.h, _ptr(root), _ptr(rnd), _ptr(pers), n))
        return root, rnd, pers, int(rounds.value), int(left.value), bool(conv.value)

    def merge_release(self):
        """free the per-label buffer of xb_merge_basins (it is kept between calls while the grid's shape stays) and the
        fetched results"""
        check(self.lib.xb_merge_release(self.h))

    def weight_sum(self, alpha, voxel_volume, q=None, use_labels=True):
        """the weight method on the resident density and labels (xb_weight_sum): `q` None integrates the resident density
        itself, a host array or a float32 / float64 device array of any strides another field of the grid's shape;
        `use_labels` False: no voxel is vacuum and the resident labels are not read (neither way are they written);
        -> (linear voxel index int64[M], charge f64[M], volume f64[M]) of the maxima in ascending voxel index"""
        self.set_option(XB_OPT_WEIGHT_NO_LABELS, 0 if use_labels else 1)
        try:
            return self._weight_sum(alpha, voxel_volume, q)
        finally:
            self.set_option(XB_OPT_WEIGHT_NO_LABELS, 0)

    def weight_release(self):
        """free the weight method's device buffers (they are kept between calls while the grid stays)"""
        check(self.lib.xb_weight_release(self.h))

    def _weight_sum(self, alpha, voxel_volume, q):
        from . import device
        al = _f64(alpha).reshape(27)
        n = C.c_int64()
        if q is not None and device.is_device_array(q):
            d = device.describe(q)
            if d.shape != self.shape:
                self._refuse_shape('weight_sum', d.shape)
            if d.dtype not in device.FLOAT_CODE:
                err = BaderHipError(f'weight_sum: dtype {d.dtype.name} is neither float32 nor float64')
                err.code = XB_E_ARG
                raise err
            st = (C.c_int64 * 3)(*d.strides)
            check(self.lib.xb_weight_sum_device(self.h, al.ctypes.data_as(_pdbl), float(voxel_volume), C.c_void_p(d.ptr),
                                                device.FLOAT_CODE[d.dtype], st, device.stream_for(d), C.byref(n)))
        else:
            if q is not None:
                q = _f64(q)
                if q.shape != self.shape:
                    self._refuse_shape('weight_sum', q.shape)
            check(self.lib.xb_weight_sum(self.h, al.ctypes.data_as(_pdbl), float(voxel_volume),
                                         None if q is None else _ptr(q), C.byref(n)))
        idx, ch, vo = np.zeros(n.value, np.int64), np.zeros(n.value, np.float64), np.zeros(n.value, np.float64)
        check(self.lib.xb_weight_fetch(self.h, _ptr(idx), _ptr(ch), _ptr(vo), n.value))
        return idx, ch, vo

    def weight_stats(self):
        """the last weight_sum: levels, how many ran as batched launches and how many in the single-workgroup tail,
        batches (host waits), voxels finished, largest batched frontier, device bytes of the method's buffers"""
        out = (C.c_int64 * 7)()
        check(self.lib.xb_weight_stats(self.h, out))
        keys = ('levels', 'levels_batched', 'levels_tail', 'batches', 'voxels', 'peak_frontier', 'bytes')
        return dict(zip(keys, (int(v) for v in out)))

    def voronoi_assign(self, lattice, atoms_cart, vac_tol=None, full_search=False, want_stats=True):
        """the resident labels become the Voronoi partition: every voxel the index of its nearest atom over the 27 periodic
        images, ties to the smaller index (xb_voronoi_assign; `lattice` the cell, a row per axis; `atoms_cart` [n, 3]); with
        `vac_tol` voxels of the resident density at or below it get -1.  `full_search`: every tile searches all images (the
        second implementation).  -> {'candidate_tiles', 'full_tiles', 'max_candidates'}, or None without `want_stats`"""
        self.drop_label_token()
        lat, at = _f64(lattice).reshape(9), _f64(atoms_cart).reshape(-1, 3)
        tol = float('nan') if vac_tol is None else float(vac_tol)
        st = (C.c_int64 * 3)()
        check(self.lib.xb_voronoi_assign(self.h, lat.ctypes.data_as(_pdbl), at.ctypes.data_as(_pdbl), at.shape[0], tol,
                                         XB_VORONOI_FULL_SEARCH if full_search else 0, st if want_stats else None))
        if want_stats:
            return dict(zip(('candidate_tiles', 'full_tiles', 'max_candidates'), (int(v) for v in st)))

    def critical_points(self, vac_tol=None, flood=False):
        """the piecewise-linear critical points of the resident density (xb_critical_points; `vac_tol`: voxels at or below it are
        neither counted nor listed; `flood`: components by flood fill instead of the table, the second implementation) ->
        (counts int64[6] indexed by XB_CRITICAL_*, lin int64[P] ascending, lower_mask uint16[P], ring uint8[P], bond uint8[P])"""
        tol = float('nan') if vac_tol is None else float(vac_tol)
        counts, n = np.zeros(XB_CRITICAL_COUNTS, np.int64), C.c_int64()
        check(self.lib.xb_critical_points(self.h, tol, XB_CRITICAL_FLOOD if flood else 0, counts.ctypes.data_as(_pi64), C.byref(n)))
        p = int(n.value)
        lin, mask = np.zeros(p, np.int64), np.zeros(p, np.uint16)
        ring, bond = np.zeros(p, np.uint8), np.zeros(p, np.uint8)
        check(self.lib.xb_critical_fetch(self.h, _ptr(lin), _ptr(mask), _ptr(ring), _ptr(bond), p))
        return counts, lin, mask, ring, bond

    def critical_bonds(self, n):
        """the bond graph of the last critical_points call on the resident labels 0 .. n - 1 (xb_critical_bonds) ->
        (pairs int32[P, 2] ascending with a < b, saddles int64[P], rho_b f64[P], voxel int64[P], same_basin)"""
        np_, same = C.c_int64(), C.c_int64()
        check(self.lib.xb_critical_bonds(self.h, int(n), C.byref(np_), C.byref(same)))
        p = int(np_.value)
        a, b = np.zeros(p, np.int32), np.zeros(p, np.int32)
        saddles, rho_b, voxel = np.zeros(p, np.int64), np.zeros(p, np.float64), np.zeros(p, np.int64)
        check(self.lib.xb_critical_bonds_fetch(self.h, _ptr(a), _ptr(b), _ptr(saddles), _ptr(rho_b), _ptr(voxel), p))
        return np.stack([a, b], axis=1), saddles, rho_b, voxel, int(same.value)

    def critical_release(self):
        """free the record list and the table of xb_critical_points (kept between calls while the grid's shape stays) and the
        fetched results"""
        check(self.lib.xb_critical_release(self.h))

    def laplacian_field(self, lattice, gather=False, on_device=False, out=None):
        """the Laplacian of the resident density at every voxel (xb_laplacian_field; `lattice` the cell, a row per axis;
        `gather`: one thread per voxel reading global memory instead of tiles in LDS, the second implementation) -> f64 of the
        grid's shape: a host array, or with `on_device` a device.DeviceArray (`out`: one to write into instead of a new one)"""
        lat = _f64(lattice).reshape(9)
        flags = XB_STENCIL_GATHER if gather else 0
        if on_device or out is not None:
            from . import device
            if out is None:
                out = device.DeviceArray(self, self.shape or (0,), np.float64)
            d, _ = self._flat('laplacian_field', out, {np.dtype(np.float64): 64}, True)
            check(self.lib.xb_laplacian_field(self.h, lat.ctypes.data_as(_pdbl), flags, None, C.c_void_p(d.ptr)))
            return out
        out = np.empty(self.shape or (0,), np.float64)
        check(self.lib.xb_laplacian_field(self.h, lat.ctypes.data_as(_pdbl), flags, _ptr(out), None))
        return out

    def laplacian_sum(self, lattice, n, voxel_volume, gather=False):
        """the Laplacian of the resident density summed over the voxels of each resident label 0 .. n - 1 (xb_laplacian_sum) ->
        (sum f64[n], sum of magnitudes f64[n], volume f64[n]), each multiplied once by voxel_volume"""
        lat, n = _f64(lattice).reshape(9), int(n)
        s, m, vo = (np.zeros(max(n, 0), np.float64) for _ in range(3))
        check(self.lib.xb_laplacian_sum(self.h, lat.ctypes.data_as(_pdbl), n, float(voxel_volume), XB_STENCIL_GATHER if gather else 0,
                                        s.ctypes.data_as(_pdbl), m.ctypes.data_as(_pdbl), vo.ctypes.data_as(_pdbl)))
        return s, m, vo

    def stencil_points(self, lattice, lin):
        """rho, its gradient (x y z) and its Hessian (xx xy xz yy yz zz) of the resident density at the linear C-order voxel
        indices `lin` (xb_stencil_points) -> f64[m, 10]"""
        lat, idx = _f64(lattice).reshape(9), np.ascontiguousarray(lin, dtype=np.int64).reshape(-1)
        out = np.zeros((idx.shape[0], XB_STENCIL_POINT_VALUES), np.float64)
        check(self.lib.xb_stencil_points(self.h, lat.ctypes.data_as(_pdbl), _ptr(idx), idx.shape[0], _ptr(out)))
        return out

    def nci_field(self, lattice, gather=False, on_device=False, out=None):
        """the reduced density gradient s and sign(lambda2) rho of the resident density at every voxel (xb_nci_field; `lattice`
        the cell, a row per axis; `gather`: the second implementation, as in laplacian_field) -> (s, x), f64 of the grid's shape
        each: host arrays, or with `on_device` two device.DeviceArray (`out`: a pair to write into instead of new ones)"""
        lat = _f64(lattice).reshape(9)
        flags = XB_STENCIL_GATHER if gather else 0
        if on_device or out is not None:
            from . import device
            if out is None:
                out = [device.DeviceArray(self, self.shape or (0,), np.float64) for _ in range(2)]
            ptr = [C.c_void_p(self._flat('nci_field', o, {np.dtype(np.float64): 64}, True)[0].ptr) for o in out]
            check(self.lib.xb_nci_field(self.h, lat.ctypes.data_as(_pdbl), flags, None, None, ptr[0], ptr[1]))
            return out[0], out[1]
        s, x = np.empty(self.shape or (0,), np.float64), np.empty(self.shape or (0,), np.float64)
        check(self.lib.xb_nci_field(self.h, lat.ctypes.data_as(_pdbl), flags, _ptr(s), _ptr(x), None, None))
        return s, x

    def nci_sum(self, lattice, n, voxel_volume, s_cut, rho_cut, rho_split, gather=False):
        """the NCI region (rho > 0, s < s_cut, rho < rho_cut) of the resident density summed over the voxels of each resident
        label 0 .. n - 1 and each class (attractive, van der Waals, repulsive by sign(lambda2) rho against rho_split)
        (xb_nci_sum) -> (count i64[n, 3], charge f64[n, 3], charge2 f64[n, 3]): the voxel count, the sums of rho and of rho^2,
        the sums multiplied once by voxel_volume"""
        lat, n = _f64(lattice).reshape(9), int(n)
        count = np.zeros((max(n, 0), 3), np.int64)
        charge, charge2 = np.zeros((max(n, 0), 3), np.float64), np.zeros((max(n, 0), 3), np.float64)
        check(self.lib.xb_nci_sum(self.h, lat.ctypes.data_as(_pdbl), n, float(voxel_volume), float(s_cut), float(rho_cut),
                                  float(rho_split), XB_STENCIL_GATHER if gather else 0, count.ctypes.data_as(_pi64),
                                  charge.ctypes.data_as(_pdbl), charge2.ctypes.data_as(_pdbl)))
        return count, charge, charge2

    def nci_hist(self, lattice, s_edges, x_edges, gather=False):
        """the histogram of the resident density's voxels with rho > 0 over the bins of s (edges `s_edges` f64[n_s + 1]) and of
        sign(lambda2) rho (`x_edges` f64[n_x + 1]) (xb_nci_hist) -> i64[n_s, n_x], exact"""
        lat = _f64(lattice).reshape(9)
        se, xe = (np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in (s_edges, x_edges))
        n_s, n_x = se.shape[0] - 1, xe.shape[0] - 1
        # (a refused bin count never reaches the allocation of its counts)
        ok = 1 <= n_s <= XB_NCI_BINS_MAX and 1 <= n_x <= XB_NCI_BINS_MAX and n_s * n_x <= XB_NCI_BINS_MAX
        counts = np.zeros((n_s, n_x) if ok else (1, 1), np.int64)
        check(self.lib.xb_nci_hist(self.h, lat.ctypes.data_as(_pdbl), se.ctypes.data_as(_pdbl), n_s, xe.ctypes.data_as(_pdbl), n_x,
                                   XB_STENCIL_GATHER if gather else 0, counts.ctypes.data_as(_pi64)))
        return counts

    def dori_field(self, lattice, rho_min, gather=False, on_device=False, colour=True, out=None):
        """DORI's gamma and, with `colour`, x = sign(lambda2) rho of the resident density at every voxel (xb_dori_field; `lattice`
        the cell, a row per axis; gamma = 0 and x = 0 where rho is not above `rho_min`; `gather`: the second implementation, as in
        laplacian_field) -> (gamma, x), f64 of the grid's shape each, x None without `colour`: host arrays, or with `on_device`
        device.DeviceArrays (`out`: a pair to write into instead of new ones, its second entry None for gamma alone)"""
        lat = _f64(lattice).reshape(9)
        flags = XB_STENCIL_GATHER if gather else 0
        if on_device or out is not None:
            from . import device
            if out is None:
                out = [device.DeviceArray(self, self.shape or (0,), np.float64) for _ in range(2 if colour else 1)] + [None]
            ptr = [None if o is None else C.c_void_p(self._flat('dori_field', o, {np.dtype(np.float64): 64}, True)[0].ptr) for o in out[:2]]
            check(self.lib.xb_dori_field(self.h, lat.ctypes.data_as(_pdbl), float(rho_min), flags, None, None, ptr[0], ptr[1]))
            return out[0], out[1]
        g = np.empty(self.shape or (0,), np.float64)
        x = np.empty(self.shape or (0,), np.float64) if colour else None
        check(self.lib.xb_dori_field(self.h, lat.ctypes.data_as(_pdbl), float(rho_min), flags, _ptr(g), None if x is None else _ptr(x),
                                     None, None))
        return g, x

    def dori_sum(self, lattice, n, voxel_volume, d_cut, rho_min, rho_split, gather=False):
        """the DORI region (gamma >= d_cut; gamma = 0 where rho is not above rho_min) of the resident density summed over the
        voxels of each resident label 0 .. n - 1 and each class (attractive, van der Waals, repulsive by sign(lambda2) rho against
        rho_split) (xb_dori_sum) -> (count i64[n, 3], charge f64[n, 3], charge2 f64[n, 3]): the voxel count, the sums of rho and
        of rho^2, the sums multiplied once by voxel_volume"""
        lat, n = _f64(lattice).reshape(9), int(n)
        count = np.zeros((max(n, 0), 3), np.int64)
        charge, charge2 = np.zeros((max(n, 0), 3), np.float64), np.zeros((max(n, 0), 3), np.float64)
        check(self.lib.xb_dori_sum(self.h, lat.ctypes.data_as(_pdbl), n, float(voxel_volume), float(d_cut), float(rho_min),
                                   float(rho_split), XB_STENCIL_GATHER if gather else 0, count.ctypes.data_as(_pi64),
                                   charge.ctypes.data_as(_pdbl), charge2.ctypes.data_as(_pdbl)))
        return count, charge, charge2

    def _field_ptr(self, what, obj):
        """the device pointer of a C-contiguous float64 device array of the grid's shape, or None for None; the context's stream
        takes up its work after everything queued so far on the stream the array belongs to (xb_stream_wait)"""
        if obj is None:
            return None
        d, stream = self._flat(what, obj, {np.dtype(np.float64): 64}, False)
        check(self.lib.xb_stream_wait(self.h, stream))
        return C.c_void_p(d.ptr)

    def isosurface(self, lattice, level, field=None, colour=None, n=0, gather=False, fetch=True):
        """marching tetrahedra on the resident density, or on `field` (a float64 device array of the grid's shape), at `level`
        (xb_isosurface + xb_isosurface_fetch; `colour`: a float64 device array interpolated onto the vertices; `n`: the resident
        labels 0 .. n - 1 share the inside volume; `gather`: the second implementation) -> (vertices f64[V, 3] in voxel
        coordinates, colour f64[V] or None, triangles i64[T, 3], wrap u16[T], cells i64[T], area, volume, volume_by_label f64[n]).
        The mesh stays on the device until isosurface_release or the next call; without `fetch` only (V, T) comes back."""
        lat, n = _f64(lattice).reshape(9), int(n)
        counts = np.zeros(2, np.int64)
        check(self.lib.xb_isosurface(self.h, self._field_ptr('isosurface', field), self._field_ptr('isosurface', colour),
                                     lat.ctypes.data_as(_pdbl), float(level), n, XB_ISO_GATHER if gather else 0, counts.ctypes.data_as(_pi64)))
        if not fetch:
            return int(counts[0]), int(counts[1])
        return self.isosurface_fetch(int(counts[0]), int(counts[1]), colour is not None, n)

    def isosurface_fetch(self, n_vertices, n_triangles, with_colour=False, n=0):
        """the mesh of the last isosurface call into host arrays of the given capacities (xb_isosurface_fetch)"""
        v, t = int(n_vertices), int(n_triangles)
        vert, col = np.zeros((v, 3), np.float64), (np.zeros(v, np.float64) if with_colour else None)
        tri, wrap, cell = np.zeros((t, 3), np.int64), np.zeros(t, np.uint16), np.zeros(t, np.int64)
        sc, vbl = np.zeros(2, np.float64), np.zeros(max(int(n), 0), np.float64)
        check(self.lib.xb_isosurface_fetch(self.h, 0, _ptr(vert), _ptr(col) if with_colour else None, _ptr(tri), _ptr(wrap), _ptr(cell), v, t,
                                           sc.ctypes.data_as(_pdbl), vbl.ctypes.data_as(_pdbl), vbl.shape[0]))
        return vert, col, tri, wrap, cell, float(sc[0]), float(sc[1]), vbl

    def isosurface_release(self):
        """free the mesh xb_isosurface keeps on the device"""
        check(self.lib.xb_isosurface_release(self.h))

    def isosurface_nci_mask(self, s, rho_cut):
        """s := ISO_NCI_RAISED wherever the resident density is >= rho_cut or s is not below it, in place on the float64 device
        array `s` (xb_isosurface_nci_mask)"""
        d, stream = self._flat('isosurface_nci_mask', s, {np.dtype(np.float64): 64}, True)
        check(self.lib.xb_stream_wait(self.h, stream))
        check(self.lib.xb_isosurface_nci_mask(self.h, C.c_void_p(d.ptr), float(rho_cut)))

    def regions_label(self, mode, field=None, level=0.0, lattice=None, s_cut=0.0, rho_cut=0.0, global_route=False, gather=False, times=False):
        """the connected components of a mask of the grid under the Freudenthal adjacency (xb_regions_label).  `mode`:
        XB_DOMAINS_ABOVE / XB_DOMAINS_BELOW (`field` >= / < `level`; `field` a float64 C-contiguous device array, None for the
        resident density) or XB_DOMAINS_NCI (the NCI region of the resident density in the cell `lattice`).  `global_route`: the
        second implementation; `gather`: the NCI predicate's values from global memory; `times`: the stages are timed with events
        (regions_times).  -> m, the number of components; the map stays on the device until regions_release"""
        lat = None if lattice is None else _f64(lattice).reshape(9)
        flags = (XB_DOMAINS_GLOBAL if global_route else 0) | (XB_DOMAINS_GATHER if gather else 0) | (XB_DOMAINS_TIMES if times else 0)
        m = C.c_int64(0)
        check(self.lib.xb_regions_label(self.h, int(mode), self._field_ptr('regions_label', field), float(level),
                                        None if lat is None else lat.ctypes.data_as(_pdbl), float(s_cut), float(rho_cut), flags, C.byref(m)))
        return int(m.value)

    def regions_sums(self, m, voxel_volume, rho_split=None):
        """per component of the last regions_label, on the resident density (xb_regions_sums) -> (seed i64[m], count i64[m], top
        i64[m], sum1 f64[m], sum2 f64[m]), and with `rho_split` (NCI components) also (count3 i64[m, 3], sum1_3 f64[m, 3], sum2_3
        f64[m, 3]); the sums multiplied once by voxel_volume"""
        m = int(m)
        seed, count, top = (np.zeros(m, np.int64) for _ in range(3))
        s1, s2 = np.zeros(m, np.float64), np.zeros(m, np.float64)
        classes = rho_split is not None
        c3, s13, s23 = np.zeros((m, 3), np.int64), np.zeros((m, 3), np.float64), np.zeros((m, 3), np.float64)
        check(self.lib.xb_regions_sums(self.h, float(voxel_volume), float(rho_split) if classes else float('nan'), seed.ctypes.data_as(_pi64),
                                       count.ctypes.data_as(_pi64), top.ctypes.data_as(_pi64), s1.ctypes.data_as(_pdbl), s2.ctypes.data_as(_pdbl),
                                       c3.ctypes.data_as(_pi64) if classes else None, s13.ctypes.data_as(_pdbl) if classes else None,
                                       s23.ctypes.data_as(_pdbl) if classes else None, m))
        return (seed, count, top, s1, s2) + ((c3, s13, s23) if classes else ())

    def regions_shares(self, n, force_list=False):
        """the voxels of every component of the last regions_label per resident label 0 .. n - 1 (xb_regions_shares +
        xb_regions_shares_fetch; `force_list`: the route of the large case) -> (component i32[t], label i32[t], count i64[t]),
        ascending in (component, label), count > 0"""
        nt = C.c_int64(0)
        check(self.lib.xb_regions_shares(self.h, int(n), XB_DOMAINS_SHARES_LIST if force_list else 0, C.byref(nt)))
        t = int(nt.value)
        comp, lab, cnt = np.zeros(t, np.int32), np.zeros(t, np.int32), np.zeros(t, np.int64)
        check(self.lib.xb_regions_shares_fetch(self.h, _ptr(comp), _ptr(lab), cnt.ctypes.data_as(_pi64), t))
        return comp, lab, cnt

    def regions_map(self, on_device=False):
        """the component of every voxel, -1 outside (xb_regions_fetch_map) -> int32 of the grid's shape: a host array, or with
        `on_device` a device.DeviceArray"""
        if on_device:
            from . import device
            out = device.DeviceArray(self, self.shape or (0,), np.int32)
            d, _ = self._flat('regions_map', out, {np.dtype(np.int32): 4}, True)
            check(self.lib.xb_regions_fetch_map(self.h, 1, C.c_void_p(d.ptr)))
            return out
        out = np.empty(self.shape or (0,), np.int32)
        check(self.lib.xb_regions_fetch_map(self.h, 0, _ptr(out)))
        return out

    def regions_times(self):
        """milliseconds of the four stages of the last regions_label(..., times=True) (xb_regions_times) -> f64[4]: membership and
        tile union-find, the unions in global memory, the flatten, the numbering"""
        ms = np.zeros(4, np.float64)
        check(self.lib.xb_regions_times(self.h, ms.ctypes.data_as(_pdbl)))
        return ms

    def regions_release(self):
        """free the map and the seeds xb_regions_label keeps on the device"""
        check(self.lib.xb_regions_release(self.h))

    def device_copy(self, host):
        """a new device.DeviceArray with the content of the host array `host` (xb_device_write)"""
        from . import device
        host = np.ascontiguousarray(host)
        out = device.DeviceArray(self, host.shape, host.dtype)
        check(self.lib.xb_device_write(self.h, C.c_void_p(out.ptr), _ptr(host), host.nbytes))
        return out

    def hirshfeld_setup(self, lattice, atoms_cart, species, tables, r_cut):
        """the cell, the atoms and the pro-atoms of the Hirshfeld calls go to the device (xb_hirshfeld_setup; `lattice` the cell, a
        row per axis; `atoms_cart` [n, 3]; `species` int[n]; `tables` f64[S, K + 1] uniform in r^2 with a last column of zeros;
        `r_cut` f64[S]).  The setup stays until the grid's shape changes or hirshfeld_release()."""
        lat, at = _f64(lattice).reshape(9), _f64(atoms_cart).reshape(-1, 3)
        sp = np.ascontiguousarray(species, dtype=np.int32).reshape(-1)
        tab, rc = _f64(tables), _f64(r_cut).reshape(-1)
        self.hirshfeld_key = None   # (whatever hirshfeld._setup remembered is no longer what the library holds)
        if tab.ndim != 2 or tab.shape[0] != rc.shape[0] or sp.shape[0] != at.shape[0]:
            raise ValueError(f'hirshfeld_setup: tables {tab.shape}, r_cut {rc.shape}, species {sp.shape}, atoms {at.shape} do not fit')
        check(self.lib.xb_hirshfeld_setup(self.h, lat.ctypes.data_as(_pdbl), at.ctypes.data_as(_pdbl), _ptr(sp), at.shape[0],
                                          tab.ctypes.data_as(_pdbl), rc.ctypes.data_as(_pdbl), rc.shape[0], tab.shape[1] - 1))
        self._hirshfeld_atoms = at.shape[0]

    def hirshfeld_release(self):
        """free the setup of hirshfeld_setup (kept while the grid's shape stays)"""
        self.hirshfeld_key = None
        check(self.lib.xb_hirshfeld_release(self.h))

    def hirshfeld_sum(self, voxel_volume, full_search=False):
        """Hirshfeld charge and volume of every atom of the setup for the resident density (xb_hirshfeld_sum) ->
        (charge f64[n], volume f64[n], rest f64[2]: charge and volume of the voxels no pro-atom reaches,
        {'candidate_tiles', 'full_tiles', 'max_candidates'})"""
        n = int(getattr(self, '_hirshfeld_atoms', 0))
        charge, volume, rest = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros(2)
        st = (C.c_int64 * 3)()
        check(self.lib.xb_hirshfeld_sum(self.h, float(voxel_volume), XB_HIRSHFELD_FULL_SEARCH if full_search else 0,
                                        charge.ctypes.data_as(_pdbl), volume.ctypes.data_as(_pdbl), rest.ctypes.data_as(_pdbl), st))
        return charge[:n], volume[:n], rest, dict(zip(('candidate_tiles', 'full_tiles', 'max_candidates'), (int(v) for v in st)))

    def hirshfeld_field(self, mode, full_search=False, on_device=False, out=None):
        """the promolecular density (mode XB_HIRSHFELD_PROMOLECULE) or the deformation density rho - P of the resident density
        (XB_HIRSHFELD_DEFORMATION) at every voxel (xb_hirshfeld_field) -> f64 of the grid's shape: a host array, or with
        `on_device` a device.DeviceArray (`out`: one to write into instead of a new one)"""
        flags = XB_HIRSHFELD_FULL_SEARCH if full_search else 0
        if on_device or out is not None:
            from . import device
            if out is None:
                out = device.DeviceArray(self, self.shape or (0,), np.float64)
            d, _ = self._flat('hirshfeld_field', out, {np.dtype(np.float64): 64}, True)
            check(self.lib.xb_hirshfeld_field(self.h, int(mode), flags, None, C.c_void_p(d.ptr)))
            return out
        out = np.empty(self.shape or (0,), np.float64)
        check(self.lib.xb_hirshfeld_field(self.h, int(mode), flags, _ptr(out), None))
        return out

    def igm_field(self, lattice, fragment, mode=XB_IGM_STOCKHOLDER, p_min=0.0, full_search=False, on_device=False, want=(True, True), out=None,
                  n_fragments=None):
        """IGM's delta-g and delta-g_inter of the current table setup (hirshfeld_setup's or isa_setup's) and the resident density at
        every voxel (xb_igm_field; `lattice` the setup's cell; `fragment` int[n], -1 .. F - 1 with F <= XB_IGM_FRAGMENTS_MAX, F = `n_fragments`,
        None: max(fragment) + 1 and at least 1; `mode` XB_IGM_PRO or XB_IGM_STOCKHOLDER; both fields are +0 where P is not above
        `p_min`) -> (dg, dgi, {'candidate_tiles', 'full_tiles', 'max_candidates'}), f64 of the grid's shape each: host arrays, or
        with `on_device` device.DeviceArrays (`out`: a pair to write into instead of new ones); a field `want` leaves out, or
        whose entry of `out` is None, is None and is not stored"""
        lat = _f64(lattice).reshape(9)
        fr = np.ascontiguousarray(fragment, dtype=np.int32).reshape(-1)
        n = int(getattr(self, '_hirshfeld_atoms', fr.shape[0]))
        if fr.shape[0] != n:
            raise ValueError(f'igm_field: {fr.shape[0]} fragments for the {n} atoms of the setup')
        nf = max(int(fr.max()) + 1 if fr.size else 1, 1) if n_fragments is None else int(n_fragments)
        flags = XB_HIRSHFELD_FULL_SEARCH if full_search else 0
        st = (C.c_int64 * 3)()
        if on_device or out is not None:
            from . import device
            if out is None:
                out = [device.DeviceArray(self, self.shape or (0,), np.float64) if w else None for w in want]
            ptr = [None if o is None else C.c_void_p(self._flat('igm_field', o, {np.dtype(np.float64): 64}, True)[0].ptr) for o in out[:2]]
            check(self.lib.xb_igm_field(self.h, lat.ctypes.data_as(_pdbl), _ptr(fr), nf, int(mode), float(p_min), flags, None, None,
                                        ptr[0], ptr[1], st))
        else:
            out = [np.empty(self.shape or (0,), np.float64) if w else None for w in want]
            check(self.lib.xb_igm_field(self.h, lat.ctypes.data_as(_pdbl), _ptr(fr), nf, int(mode), float(p_min), flags,
                                        None if out[0] is None else _ptr(out[0]), None if out[1] is None else _ptr(out[1]), None, None, st))
        return out[0], out[1], dict(zip(('candidate_tiles', 'full_tiles', 'max_candidates'), (int(v) for v in st)))

    def igm_sum(self, val, x, n, voxel_volume, cut, rho_split):
        """the region val >= cut of the device field `val` (f64 of the grid's shape; `x` likewise: the class by x against rho_split,
        as nci_sum's) summed over the voxels of each resident label 0 .. n - 1 and each class (xb_igm_sum) ->
        (count i64[n, 3], charge f64[n, 3], integral f64[n, 3]): the voxel count, the sums of the resident density and of val, the
        sums multiplied once by voxel_volume"""
        n = int(n)
        count = np.zeros((max(n, 0), 3), np.int64)
        charge, integral = np.zeros((max(n, 0), 3), np.float64), np.zeros((max(n, 0), 3), np.float64)
        check(self.lib.xb_igm_sum(self.h, self._field_ptr('igm_sum', val), self._field_ptr('igm_sum', x), n, float(voxel_volume),
                                  float(cut), float(rho_split), count.ctypes.data_as(_pi64), charge.ctypes.data_as(_pdbl),
                                  integral.ctypes.data_as(_pdbl)))
        return count, charge, integral

    def isa_setup(self, lattice, atoms_cart, r_cut, shells, rho_bound, initial=None):
        """the cell, the atoms and the starting tables of the iterative stockholder atoms go to the device and the shells are
        counted (xb_isa_setup; `r_cut` f64[n], `shells` = K, `initial` None or f64[n, K], `rho_bound` >= max |rho|).  It IS the
        context's Hirshfeld setup: hirshfeld_sum / hirshfeld_field / hirshfeld_release serve it, hirshfeld_setup replaces it.
        -> {'e', 'cmax', 'pairs', 'empty_shells'}"""
        lat, at = _f64(lattice).reshape(9), _f64(atoms_cart).reshape(-1, 3)
        rc = _f64(r_cut).reshape(-1)
        self.hirshfeld_key = None   # (whatever hirshfeld._setup remembered is no longer what the library holds)
        if rc.shape[0] != at.shape[0]:
            raise ValueError(f'isa_setup: r_cut {rc.shape} for atoms {at.shape}')
        ini = None
        if initial is not None:
            ini = _f64(initial)
            if ini.shape != (at.shape[0], int(shells)):
                raise ValueError(f'isa_setup: initial tables {ini.shape}, ({at.shape[0]}, {int(shells)}) is wanted')
        info = (C.c_int64 * 4)()
        check(self.lib.xb_isa_setup(self.h, lat.ctypes.data_as(_pdbl), at.ctypes.data_as(_pdbl), at.shape[0], rc.ctypes.data_as(_pdbl),
                                    int(shells), None if ini is None else ini.ctypes.data_as(_pdbl), float(rho_bound), info))
        self._hirshfeld_atoms = at.shape[0]
        self._isa_shells = int(shells)
        return dict(zip(('e', 'cmax', 'pairs', 'empty_shells'), (int(v) for v in info)))

    def isa_iterate(self, iters=1, direct=False, full_search=False):
        """`iters` iterations of the setup's tables on the resident density, one host wait (xb_isa_iterate) ->
        (qsum i64[iters, n]: every iteration's fixed-point charges, {'candidate_tiles', 'full_tiles', 'max_candidates', 'beyond_bound'})"""
        n = int(getattr(self, '_hirshfeld_atoms', 0))
        qsum = np.zeros((max(int(iters), 1), max(n, 1)), np.int64)
        st = (C.c_int64 * 4)()
        flags = (XB_ISA_DIRECT if direct else 0) | (XB_HIRSHFELD_FULL_SEARCH if full_search else 0)
        check(self.lib.xb_isa_iterate(self.h, int(iters), flags, qsum.ctypes.data_as(_pi64), st))
        return qsum[:, :n], dict(zip(('candidate_tiles', 'full_tiles', 'max_candidates', 'beyond_bound'), (int(v) for v in st)))

    def isa_tables(self):
        """the current tables and the shell counts of the ISA setup (xb_isa_tables) -> (A f64[n, K], count i64[n, K])"""
        n, K = int(getattr(self, '_hirshfeld_atoms', 0)), int(getattr(self, '_isa_shells', 0))
        A, count = np.zeros((max(n, 1), max(K, 1))), np.zeros((max(n, 1), max(K, 1)), np.int64)
        check(self.lib.xb_isa_tables(self.h, A.ctypes.data_as(_pdbl), count.ctypes.data_as(_pi64)))
        return A[:n, :K], count[:n, :K]

    def isa_load(self, tables):
        """f64[n, K] replace the current tables of the ISA setup; the counts and the exponent stay (xb_isa_load)"""
        n, K = int(getattr(self, '_hirshfeld_atoms', 0)), int(getattr(self, '_isa_shells', 0))
        tab = _f64(tables)
        if tab.shape != (n, K):
            raise ValueError(f'isa_load: tables {tab.shape}, ({n}, {K}) is wanted')
        check(self.lib.xb_isa_load(self.h, tab.ctypes.data_as(_pdbl)))

    def mbis_setup(self, lattice, atoms_cart, r_cut, shells, etable, knots_per_unit, init_N, init_sigma, rho_bound, voxel_volume):
        """the cell, the atoms, the exp table and the starting shells of the minimal-basis iterative stockholder atoms go to the
        device and the pairs are counted (xb_mbis_setup; `r_cut` f64[n], `shells` int[n] in 1 .. 8, `etable` f64[KE + 1] with
        E[k] = exp(-k / knots_per_unit) and a last 0, `init_N`, `init_sigma` f64[n, M], M = max shells).  It replaces the context's
        Hirshfeld or ISA setup and the reverse.  -> {'eN', 'eS', 'eV', 'eR', 'cmax', 'pairs'}"""
        lat, at = _f64(lattice).reshape(9), _f64(atoms_cart).reshape(-1, 3)
        rc, tab = _f64(r_cut).reshape(-1), _f64(etable).reshape(-1)
        sh = np.ascontiguousarray(shells, dtype=np.int32).reshape(-1)
        self.hirshfeld_key = None   # (whatever hirshfeld._setup remembered is no longer what the library holds)
        if rc.shape[0] != at.shape[0] or sh.shape[0] != at.shape[0]:
            raise ValueError(f'mbis_setup: r_cut {rc.shape}, shells {sh.shape} for atoms {at.shape}')
        M = int(sh.max()) if sh.size else 0
        N0, s0 = _f64(init_N), _f64(init_sigma)
        if N0.shape != (at.shape[0], M) or s0.shape != N0.shape:
            raise ValueError(f'mbis_setup: initial shells {N0.shape}, {s0.shape}, ({at.shape[0]}, {M}) is wanted')
        info = (C.c_int64 * 6)()
        check(self.lib.xb_mbis_setup(self.h, lat.ctypes.data_as(_pdbl), at.ctypes.data_as(_pdbl), at.shape[0], rc.ctypes.data_as(_pdbl),
                                     _ptr(sh), tab.ctypes.data_as(_pdbl), int(knots_per_unit), tab.shape[0] - 1,
                                     N0.ctypes.data_as(_pdbl), s0.ctypes.data_as(_pdbl), float(rho_bound), float(voxel_volume), info))
        self._hirshfeld_atoms = at.shape[0]
        self._mbis_stride = M
        return dict(zip(('eN', 'eS', 'eV', 'eR', 'cmax', 'pairs'), (int(v) for v in info)))

    def mbis_iterate(self, iters=1, direct=False, full_search=False, keep=False):
        """`iters` iterations of the setup's shells on the resident density, one host wait (xb_mbis_iterate; `keep`: one pass that
        leaves the parameters) -> (qsum i64[iters, n], vsum i64[iters, n], rest i64[iters, 2],
        {'candidate_tiles', 'full_tiles', 'max_candidates', 'beyond_bound'})"""
        n, k = int(getattr(self, '_hirshfeld_atoms', 0)), max(int(iters), 1)
        qsum, vsum, rest = np.zeros((k, max(n, 1)), np.int64), np.zeros((k, max(n, 1)), np.int64), np.zeros((k, 2), np.int64)
        st = (C.c_int64 * 4)()
        flags = (XB_MBIS_DIRECT if direct else 0) | (XB_HIRSHFELD_FULL_SEARCH if full_search else 0) | (XB_MBIS_KEEP if keep else 0)
        check(self.lib.xb_mbis_iterate(self.h, int(iters), flags, qsum.ctypes.data_as(_pi64), vsum.ctypes.data_as(_pi64),
                                       rest.ctypes.data_as(_pi64), st))
        return qsum[:, :n], vsum[:, :n], rest, dict(zip(('candidate_tiles', 'full_tiles', 'max_candidates', 'beyond_bound'), (int(v) for v in st)))

    def mbis_params(self):
        """the current shells and the pair counts of the MBIS setup (xb_mbis_params) -> (N f64[n, M], sigma f64[n, M], count i64[n])"""
        n, M = int(getattr(self, '_hirshfeld_atoms', 0)), int(getattr(self, '_mbis_stride', 0))
        N, sg, count = np.zeros((max(n, 1), max(M, 1))), np.zeros((max(n, 1), max(M, 1))), np.zeros(max(n, 1), np.int64)
        check(self.lib.xb_mbis_params(self.h, N.ctypes.data_as(_pdbl), sg.ctypes.data_as(_pdbl), count.ctypes.data_as(_pi64)))
        return N[:n, :M], sg[:n, :M], count[:n]

    def mbis_load(self, N, sigma):
        """f64[n, M] populations and widths replace the current shells of the MBIS setup (xb_mbis_load)"""
        n, M = int(getattr(self, '_hirshfeld_atoms', 0)), int(getattr(self, '_mbis_stride', 0))
        N, sg = _f64(N), _f64(sigma)
        if N.shape != (n, M) or sg.shape != (n, M):
            raise ValueError(f'mbis_load: shells {N.shape}, {sg.shape}, ({n}, {M}) is wanted')
        check(self.lib.xb_mbis_load(self.h, N.ctypes.data_as(_pdbl), sg.ctypes.data_as(_pdbl)))

    def mbis_field(self, mode, full_search=False, on_device=False, out=None):
        """the sum of the MBIS pro-atoms (mode XB_HIRSHFELD_PROMOLECULE) or the resident density minus it (XB_HIRSHFELD_DEFORMATION)
        at every voxel (xb_mbis_field) -> f64 of the grid's shape: a host array, or with `on_device` a device.DeviceArray"""
        flags = XB_HIRSHFELD_FULL_SEARCH if full_search else 0
        if on_device or out is not None:
            from . import device
            if out is None:
                out = device.DeviceArray(self, self.shape or (0,), np.float64)
            d, _ = self._flat('mbis_field', out, {np.dtype(np.float64): 64}, True)
            check(self.lib.xb_mbis_field(self.h, int(mode), flags, None, C.c_void_p(d.ptr)))
            return out
        out = np.empty(self.shape or (0,), np.float64)
        check(self.lib.xb_mbis_field(self.h, int(mode), flags, _ptr(out), None))
        return out

    def stockholder_moments(self, rho_bound, direct=False, full_search=False):
        """the twelve integer sums per atom of the current setup -- Hirshfeld, ISA or MBIS -- on the resident density, one host wait
        (xb_stockholder_moments; `rho_bound` >= max |rho|) -> (bins i64[n, 12], {'E': (E0 .. E4), 'cmax', 'pairs', 'beyond_bound'},
        {'candidate_tiles', 'full_tiles', 'max_candidates'})"""
        n = int(getattr(self, '_hirshfeld_atoms', 0))
        bins = np.zeros((max(n, 1), 12), np.int64)
        info, st = (C.c_int64 * 8)(), (C.c_int64 * 3)()
        flags = (XB_STOCKMOM_DIRECT if direct else 0) | (XB_HIRSHFELD_FULL_SEARCH if full_search else 0)
        check(self.lib.xb_stockholder_moments(self.h, float(rho_bound), flags, bins.ctypes.data_as(_pi64), info, st))
        v = [int(x) for x in info]
        return (bins[:n], {'E': tuple(v[:5]), 'cmax': v[5], 'pairs': v[6], 'beyond_bound': v[7]},
                dict(zip(('candidate_tiles', 'full_tiles', 'max_candidates'), (int(x) for x in st))))

    def density_absmax(self):
        """max |rho| of the resident density (xb_isa_rho_bound)"""
        out = C.c_double()
        check(self.lib.xb_isa_rho_bound(self.h, C.byref(out)))
        return float(out.value)

    def volume_assign(self, swap):
        self.drop_label_token()
        sw = np.ascontiguousarray(swap, dtype=np.int64)
        check(self.lib.xb_volume_assign(self.h, _ptr(sw), sw.shape[0]))

    def surface_distance(self, lattice, atoms_cart):
        lat, at = _f64(lattice).reshape(9), _f64(atoms_cart).reshape(-1, 3)
        out = np.zeros(at.shape[0], np.float64)
        e = C.c_int64()
        check(self.lib.xb_surface_distance(self.h, _ptr(lat), _ptr(at), at.shape[0], _ptr(out), C.byref(e)))
        return out, e.value

    def volume_mask(self, vol_num):
        out = np.empty(self.shape, np.float64)
        check(self.lib.xb_volume_mask(self.h, int(vol_num), _ptr(out)))
        return out

    def label_sum(self, value):
        s, n = C.c_double(), C.c_int64()
        check(self.lib.xb_label_sum(self.h, int(value), C.byref(s), C.byref(n)))
        return s.value, n.value

    def set_table_window(self, margin):
        check(self.lib.xb_set_table_window(self.h, int(margin)))

    def table_build(self):
        n = C.c_int64()
        check(self.lib.xb_table_build(self.h, C.byref(n)))
        out = np.zeros(n.value, np.int64)
        check(self.lib.xb_table_local_seeds(self.h, _ptr(out), n.value))
        return out

    def brick_masks(self):
        p, n, f, k = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.xb_brick_masks(self.h, C.byref(p), C.byref(n), C.byref(f), C.byref(k)))
        return p.value, n.value, f.value, k.value

    def table_ties(self):
        t = C.c_int64()
        check(self.lib.xb_table_ties(self.h, C.byref(t)))
        return bool(t.value)

    def table_finish(self, seeds, any_ties=True):
        sd = np.ascontiguousarray(seeds, dtype=np.int64)
        check(self.lib.xb_table_finish(self.h, _ptr(sd), sd.shape[0], int(bool(any_ties))))

    def copy_planes(self, which, to_device, host, xa, xb):
        self.drop_label_token()
        check(self.lib.xb_copy_planes(self.h, int(which), int(to_device), _ptr(host), int(xa), int(xb)))

    # -- measurement ------------------------------------------------------------------------
    def plane_elems(self):
        return int(self.lib.xb_plane_elems(self.h))

    def brick_masks_copy(self, host, first, count):
        """the chunk [first, first+count) of the per-brick move masks: host=None downloads it, else uploads `host`"""
        if host is None:
            out = np.empty(2 * int(count), np.int32)     # the masks, then the bricks' single-maximum voxels
            check(self.lib.xb_brick_masks_copy(self.h, 0, _ptr(out), int(first), int(count)))
            return out
        buf = np.ascontiguousarray(host, np.int32)
        assert buf.size == 2 * int(count)
        check(self.lib.xb_brick_masks_copy(self.h, 1, _ptr(buf), int(first), int(count)))

    # -- multi-GPU transport (csrc/comm.h: RCCL through the C ABI) ---------------------------------
    def comm_unique_id(self):
        buf = np.zeros(128, np.uint8)
        check(self.lib.xb_comm_unique_id(_ptr(buf)))
        return buf.tobytes()

    def comm_init(self, rank, size, unique_id):
        buf = np.frombuffer(unique_id, np.uint8).copy()
        assert buf.size == 128
        check(self.lib.xb_comm_init(self.h, int(rank), int(size), _ptr(buf)))
        self.comm_size = int(size)

    def comm_allreduce(self, vals, op='sum'):
        a = np.array([int(v) for v in vals], np.int64)
        check(self.lib.xb_comm_allreduce_i64(self.h, a.ctypes.data_as(_pi64), a.size, {'sum': 0, 'min': 1, 'max': 2}[op]))
        return a.tolist()

    def comm_allgather(self, vals, size=None):
        a = np.ascontiguousarray(vals, np.int64).reshape(-1)
        n = int(self.comm_size if size is None else size)
        out = np.empty(n * a.size, np.int64)
        check(self.lib.xb_comm_allgather_i64(self.h, a.ctypes.data_as(_pi64), a.size, out.ctypes.data_as(_pi64)))
        return out

    def comm_exchange_planes(self, which, sends, recvs):
        self.drop_label_token()
        def cols(ops):
            peer = np.array([o[0] for o in ops], np.int32)
            xa = np.array([o[1] for o in ops], np.int64)
            xb = np.array([o[2] for o in ops], np.int64)
            return peer, xa, xb
        sp, sa, sb = cols(sends)
        rp, ra, rb = cols(recvs)
        check(self.lib.xb_comm_exchange_planes(self.h, int(which), len(sends), _ptr(sp), sa.ctypes.data_as(_pi64),
                                               sb.ctypes.data_as(_pi64), len(recvs), _ptr(rp), ra.ctypes.data_as(_pi64),
                                               rb.ctypes.data_as(_pi64)))

    def comm_share_brick_masks(self, first, count):
        f, n = np.array(first, np.int64), np.array(count, np.int64)
        check(self.lib.xb_comm_share_brick_masks(self.h, f.ctypes.data_as(_pi64), n.ctypes.data_as(_pi64)))

    # ---- the slab step with its control flow on the device (csrc/slab_step.h) ----
    def slab_supported(self, nranks):
        a = C.c_int64(0)
        check(self.lib.xb_slab_supported(self.h, int(nranks), C.byref(a)))
        return bool(a.value)

    def slab_assign_masks(self, rank, nranks):
        check(self.lib.xb_slab_assign_masks(self.h, int(rank), int(nranks)))

    def slab_assign_trace(self):
        self.drop_label_token()
        check(self.lib.xb_slab_assign_trace(self.h))

    def slab_assign_finish(self):
        """-> (n_maxima, status): 0 done, 1 repeat the step, 2 use the host-driven calls"""
        self.drop_label_token()
        a, b = C.c_int64(0), C.c_int64(0)
        check(self.lib.xb_slab_assign_finish(self.h, C.byref(a), C.byref(b)))
        if b.value == 0:
            self.n_maxima = int(a.value)
        return int(a.value), int(b.value)

    def slab_refine_pass(self):
        self.drop_label_token()
        check(self.lib.xb_slab_refine_pass(self.h))

    def slab_walkers_round(self, src, last):
        self.drop_label_token()
        check(self.lib.xb_slab_walkers_round(self.h, int(src), 1 if last else 0))

    def slab_walk_send(self, walkers):
        """how many walkers of a rank's part travel in the gather of the next passes (0: the capacity); the same value on every rank"""
        check(self.lib.xb_slab_walk_send(self.h, int(walkers)))

    def slab_walk_layout(self):
        """(part bytes, header + walkers of round 0, header + walkers of later rounds, results offset, results bytes)"""
        out = np.zeros(5, np.int64)
        check(self.lib.xb_slab_walk_layout(self.h, out.ctypes.data_as(_pi64)))
        return [int(v) for v in out]

    def slab_refine_counts(self):
        """-> (local, summed): int64[XB_XC_COUNT] each, indexed by the XB_XC_* constants"""
        loc, glo = np.zeros(XB_XC_COUNT, np.int64), np.zeros(XB_XC_COUNT, np.int64)
        check(self.lib.xb_slab_refine_counts(self.h, loc.ctypes.data_as(_pi64), glo.ctypes.data_as(_pi64)))
        return loc, glo

    def slab_block(self, which):
        """(device pointer, bytes, offset of this rank's part, its bytes) of exchange block `which`"""
        p, a, b, d = _vp(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(self.lib.xb_slab_block(self.h, int(which), C.byref(p), C.byref(a), C.byref(b), C.byref(d)))
        return int(p.value or 0), int(a.value), int(b.value), int(d.value)

    def slab_block_copy(self, which, host, off, to_device):
        """bytes [off, off + host.nbytes) of block `which` from (to_device) or into the uint8 array `host`"""
        assert host.dtype == np.uint8 and host.flags.c_contiguous
        check(self.lib.xb_slab_block_copy(self.h, int(which), 1 if to_device else 0, _ptr(host), int(off), host.nbytes))

    def comm_allgather_block(self, which, first, count):
        f, n = np.array(first, np.int64), np.array(count, np.int64)
        check(self.lib.xb_comm_allgather_block(self.h, int(which), f.ctypes.data_as(_pi64), n.ctypes.data_as(_pi64)))

    def comm_allreduce_block(self):
        check(self.lib.xb_comm_allreduce_block(self.h))

    def host_waits(self):
        """waits of the host for the card inside library calls made by this thread"""
        a = C.c_int64(0)
        check(self.lib.xb_host_waits(C.byref(a)))
        return int(a.value)

    def memory_stats(self):
        """(total, table, scratch) device bytes this context holds for the grid"""
        a, b, d = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(self.lib.xb_memory_stats(self.h, C.byref(a), C.byref(b), C.byref(d)))
        return int(a.value), int(b.value), int(d.value)

    def comm_info(self):
        """{ranks, rank, device, rccl_version} as the RCCL communicator itself reports them (-1: not available)"""
        out = (C.c_int64 * 4)()
        check(self.lib.xb_comm_info(self.h, out))
        return {'nccl_comm_count': int(out[0]), 'nccl_user_rank': int(out[1]), 'nccl_device': int(out[2]), 'rccl_version': int(out[3])}

    def comm_bytes_sent(self):
        n = C.c_int64(0)
        check(self.lib.xb_comm_stats(self.h, C.byref(n)))
        return int(n.value)

    def enable_timing(self, on=True, only=None):
        """on: all timers; only=[k, ...]: just these (XB_TIMER_* constants)"""
        mask = int(bool(on)) if only is None else sum(2 << int(k) for k in only)
        check(self.lib.xb_enable_timing(self.h, mask))

    def kernel_time(self, which):
        """-> (milliseconds, launches) of timer `which` (an XB_TIMER_* constant) since the last reset"""
        ms, n = C.c_double(), C.c_int64()
        check(self.lib.xb_kernel_time(self.h, int(which), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_time_reset(self):
        check(self.lib.xb_kernel_time_reset(self.h))

    def set_option(self, key, value):
        """key: an XB_OPT_* constant; value: what the key's comment in include/bader_hip.h states"""
        check(self.lib.xb_set_option(self.h, int(key), int(value)))

    def box_stats(self):
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_box_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def brick_labels(self):
        """per 8^3 brick of the last neargrid assignment: the trapping region it was certified for (> 0) or 0 (walked)"""
        dims = (C.c_int64 * 3)()
        check(self.lib.xb_brick_labels(self.h, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), np.int32)
        check(self.lib.xb_brick_labels(self.h, _ptr(out), out.size, dims))
        return out

    def slow_path_stats(self):
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_slow_path_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def growth_stats(self):
        """(assignments repeated with the long kill schedule, kill launches scheduled now)"""
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_growth_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def deferred_stats(self):
        a = C.c_int64()
        check(self.lib.xb_deferred_stats(self.h, C.byref(a)))
        return a.value

    def sweep_stats(self):
        """(edge sweeps launched by row bit masks, by the per-voxel kernels) since the context was made"""
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_sweep_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def retrace_stats(self):
        """(first retraces of an edge list launched as the lean kernel, as the generic kernel) since the context was made"""
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_retrace_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def trace_stats(self):
        """(group traces launched with the packed neighbour-bits walker, the lean walker with the brick-label lookup, the generic
        walker) since the context was made"""
        a, b, g = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.xb_trace_stats(self.h, C.byref(a), C.byref(b), C.byref(g), None))
        return a.value, b.value, g.value

    def trace_offset_stats(self):
        """(group traces launched with a lean walker that forms 32-bit table offsets, with one that forms 64-bit offsets -- a table
        of more than 2^27 voxels) since the context was made; together the first two entries of trace_stats()"""
        a, b, w = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.xb_trace_stats(self.h, C.byref(a), C.byref(b), None, C.byref(w)))
        return a.value + b.value - w.value, w.value

    def axis_limits(self):
        """(the longest x axis, the longest y axis) set_grid accepts on this device: the tile launches' gridDim.z / gridDim.y"""
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.xb_axis_limits(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def retrace_overflow(self):
        """the voxels the retraces put on their overflow lists since the last call (DEBUG_KEEP_RETRACE_OVERFLOW set), taken"""
        n = C.c_int64()
        check(self.lib.xb_retrace_overflow(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        if n.value:
            check(self.lib.xb_retrace_overflow(self.h, _ptr(out), out.size, C.byref(n)))
        return out

    def edge_list(self):
        """(the edge list the last edge_find() left, in the sweep's order; tiles the sweep listed, -1 without a tile list)"""
        n, t = C.c_int64(), C.c_int64()
        check(self.lib.xb_edge_list(self.h, None, 0, C.byref(n), C.byref(t)))
        out = np.zeros(n.value, np.int32)
        if n.value:
            check(self.lib.xb_edge_list(self.h, _ptr(out), out.size, C.byref(n), C.byref(t)))
        return out, t.value

    def sync(self):
        check(self.lib.xb_sync(self.h))


def critical_lut():
    """xb_critical_lut: ring | bond << 4 for each of the 16 384 lower masks (host only: needs the library, not a GPU)"""
    out = np.zeros(XB_CRITICAL_LUT_SIZE, np.uint8)
    check(load().xb_critical_lut(_ptr(out)))
    return out


def isosurface_table():
    """xb_isosurface_table: uint8[6, 16, 8] -- per tetrahedron and inside mask the number of triangles and their corners as
    (owner corner of the cube) << 3 | k, 255 where unused (host only: needs the library, not a GPU)"""
    out = np.zeros(XB_ISO_TABLE_SIZE, np.uint8)
    check(load().xb_isosurface_table(_ptr(out)))
    return out.reshape(6, 16, 8)


def hirshfeld_images(lattice, atoms_cart, species, r_cut):
    """xb_hirshfeld_images: the canonical image list of the Hirshfeld calls for the cell `lattice` (a row per axis), the atoms
    [n, 3], their species int[n] and the cutoffs f64[S] -> int32[m, 4] rows (atom, x, y, z) (host only: needs the library, not a
    GPU)"""
    lat, at = _f64(lattice).reshape(9), _f64(atoms_cart).reshape(-1, 3)
    sp, rc = np.ascontiguousarray(species, dtype=np.int32).reshape(-1), _f64(r_cut).reshape(-1)
    if sp.shape[0] != at.shape[0]:
        raise ValueError(f'hirshfeld_images: {sp.shape[0]} species for {at.shape[0]} atoms')
    lib, m = load(), C.c_int64()
    args = (lat.ctypes.data_as(_pdbl), at.ctypes.data_as(_pdbl), _ptr(sp), at.shape[0], rc.ctypes.data_as(_pdbl), rc.shape[0])
    check(lib.xb_hirshfeld_images(*args, C.byref(m), None, 0))
    out = np.zeros((int(m.value), 4), np.int32)
    check(lib.xb_hirshfeld_images(*args, C.byref(m), _ptr(out), out.shape[0]))
    return out


def stencil_coeffs(lattice, shape):
    """xb_stencil_coeffs: the 51 coefficients of the stencil for the cell `lattice` (a row per axis) on a grid of `shape` ->
    (t f64[3, 3] gradient, w f64[6] Laplacian, h f64[6, 6] Hessian); host only: needs the library, not a GPU"""
    lat = _f64(lattice).reshape(9)
    out = np.zeros(XB_STENCIL_COEFFS, np.float64)
    nx, ny, nz = (int(s) for s in shape)
    check(load().xb_stencil_coeffs(lat.ctypes.data_as(_pdbl), nx, ny, nz, out.ctypes.data_as(_pdbl)))
    return out[:9].reshape(3, 3), out[9:15], out[15:].reshape(6, 6)


def atom_assign(bader_max_cart, atoms_cart, lattice):
    """utils.atom_assign (utils.py:185-232) through the C ABI (host-side, tiny)."""
    lib = load()
    bm, at, lat = _f64(bader_max_cart).reshape(-1, 3), _f64(atoms_cart).reshape(-1, 3), _f64(lattice).reshape(9)
    a, d = np.zeros(bm.shape[0], np.int64), np.zeros(bm.shape[0], np.float64)
    check(lib.xb_atom_assign(_ptr(bm), bm.shape[0], _ptr(at), at.shape[0], _ptr(lat), _ptr(a), _ptr(d)))
    return a, d


_default_ctx = {}


def default_context(device=None):
    """Process-wide context (one per device), created on first use."""
    if device is None:
        device = int(os.environ.get('PYBADER_AMD_DEVICE', os.environ.get('LOCAL_RANK', '0')))
        if load().xb_device_count() == 1:
            device = 0
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
