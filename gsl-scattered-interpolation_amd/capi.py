"""ctypes bindings of include/gsl_sinterp.h and include/gsl_sinterp_hip.h.

Mirrors the C structs (LP64) and wraps the entry points with numpy / torch
friendly helpers.  Device pointers are plain integers (``tensor.data_ptr()``).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

GSL_SUCCESS, GSL_FAILURE = 0, -1
GSL_EDOM, GSL_EFAULT, GSL_EINVAL, GSL_EFAILED, GSL_ENOMEM = 1, 3, 4, 5, 8
GSL_EBADLEN, GSL_ENOTSQR, GSL_EUNSUP, GSL_EUNIMPL = 19, 20, 23, 24
GSL_EMAXITER = 11
RBF_GAUSSIAN, RBF_TPS, RBF_WENDLAND = 0, 1, 2
RBF_MATERN32, RBF_MATERN52, RBF_IMQ = 3, 4, 5
FIT_LOO, FIT_ML = 0, 1
VARIOGRAM_MATHERON, VARIOGRAM_CRESSIE = 0, 1
VARIOGRAM_W_COUNT, VARIOGRAM_W_COUNT_H2, VARIOGRAM_W_NONE = 0, 1, 2
SOLVER_DEFAULT, SOLVER_CHOLESKY2, SOLVER_PCHOLESKY, SOLVER_LU_REFINE = 0, 1, 2, 3
TREE_DEFAULT, TREE_NOSTANDARDIZE, TREE_ISOSCALE = 0, 1, 2
TREE_RECORD_BYTES, TREE_LEAFTAB_BYTES = 64, 32
CUBIC_RECORD_BYTES = 160                              # Clough-Tocher records (n_tri of them)
NATURAL_RECORD_BYTES, NATURAL_STACK = 80, 16          # natural-neighbour records (n_tri + 1 of them); pending-stack default


def library_path():
    """The product library.  GSL_SINTERP_LIBRARY points the bindings at another BUILD of the same
    sources (the sanitizer build `make asan` of the host C, tests/test_sanitizers.py) -- never at a
    different implementation: there is no CPU fallback behind this switch."""
    return os.environ.get("GSL_SINTERP_LIBRARY") or os.path.join(_HERE, "libgsl_sinterp.so")


_lib = None


def lib():
    """Load libgsl_sinterp.so; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise ImportError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no pure-Python or CPU fallback)")
        _lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        _declare(_lib)
        _lib.gsl_set_error_handler_off()
    return _lib


# ------------------------------------------------------------------ structs
class gsl_block(C.Structure):
    _fields_ = [("size", C.c_size_t), ("data", C.POINTER(C.c_double))]


class gsl_vector(C.Structure):
    _fields_ = [("size", C.c_size_t), ("stride", C.c_size_t), ("data", C.POINTER(C.c_double)),
                ("block", C.POINTER(gsl_block)), ("owner", C.c_int)]


class gsl_matrix(C.Structure):
    _fields_ = [("size1", C.c_size_t), ("size2", C.c_size_t), ("tda", C.c_size_t),
                ("data", C.POINTER(C.c_double)), ("block", C.POINTER(gsl_block)), ("owner", C.c_int)]


class gsl_permutation(C.Structure):
    _fields_ = [("size", C.c_size_t), ("data", C.POINTER(C.c_size_t))]


class simplex_tree_node(C.Structure):
    _fields_ = [("points", C.c_int), ("links", C.c_int), ("type", C.c_uint, 2)]


class simplex_tree_accel(C.Structure):
    _fields_ = [("simplex_matrix", C.POINTER(gsl_matrix)), ("perm", C.POINTER(gsl_permutation)),
                ("coords", C.POINTER(gsl_vector)), ("current_simplex", C.c_int)]


class simplex_tree(C.Structure):
    _fields_ = [
        ("n_simplexes", C.c_int), ("max_simplexes", C.c_int), ("simplexes", C.POINTER(simplex_tree_node)),
        ("n_pidx", C.c_int), ("max_pidx", C.c_int), ("pidx", C.POINTER(C.c_int)),
        ("n_links", C.c_int), ("max_links", C.c_int), ("links", C.POINTER(C.c_int)),
        ("seed_points", C.POINTER(gsl_matrix)), ("n_points", C.c_int), ("max_points", C.c_int), ("dim", C.c_int),
        ("shift", C.POINTER(gsl_vector)), ("scale", C.POINTER(gsl_vector)),
        ("min", C.POINTER(gsl_vector)), ("max", C.POINTER(gsl_vector)),
        ("shuffle", C.POINTER(gsl_permutation)), ("accel", C.POINTER(simplex_tree_accel)),
        ("new_simplexes", C.POINTER(C.c_int)), ("old_neighbors1", C.POINTER(C.c_int)),
        ("old_neighbors2", C.POINTER(C.c_int)), ("left_out", C.POINTER(C.c_int)),
        ("tmp_points1", C.POINTER(C.c_int)), ("tmp_vec1", C.POINTER(gsl_vector)),
        ("tmp_vec2", C.POINTER(gsl_vector)), ("tmp_mat", C.POINTER(gsl_matrix)),
    ]


class gsl_sinterp(C.Structure):
    _fields_ = [("type", C.c_void_p), ("dim", C.c_size_t), ("size", C.c_size_t), ("device", C.c_int),
                ("shape", C.c_double), ("init_flags", C.c_int), ("rng", C.c_void_p), ("state", C.c_void_p),
                ("n_devices", C.c_int), ("devices", C.c_int * 64), ("solver", C.c_int), ("want_rcond", C.c_int),
                ("rcond", C.c_double), ("route", C.c_int), ("nugget", C.c_double), ("want_variance", C.c_int),
                ("want_loo", C.c_int), ("neighbours", C.c_size_t)]
    # the C struct ends with `int drift` behind these: the library allocates every gsl_sinterp, the bindings read the order
    # through gsl_sinterp_drift


_vp, _i, _sz, _d = C.c_void_p, C.c_int, C.c_size_t, C.c_double
_pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
_pm, _pv, _pt = C.POINTER(gsl_matrix), C.POINTER(gsl_vector), C.POINTER(simplex_tree)

# name -> (restype, argtypes); this table is also what tests check the .so exports
SIGNATURES = {
    # --- include/gsl_sinterp_hip.h
    "gsl_sinterp_hip_device_count": (_i, []),
    "gsl_sinterp_hip_ctx_create": (_i, [C.POINTER(_vp), _i, _vp]),
    "gsl_sinterp_hip_ctx_own_stream": (_i, [_vp]),
    "gsl_sinterp_hip_ctx_destroy": (None, [_vp]),
    "gsl_sinterp_hip_sync": (_i, [_vp]),
    "gsl_sinterp_hip_last_error": (C.c_char_p, [_vp]),
    "gsl_sinterp_hip_malloc": (_i, [_vp, C.POINTER(_vp), _sz]),
    "gsl_sinterp_hip_free": (_i, [_vp, _vp]),
    "gsl_sinterp_hip_h2d": (_i, [_vp, _vp, _vp, _sz]),
    "gsl_sinterp_hip_d2h": (_i, [_vp, _vp, _vp, _sz]),
    "gsl_sinterp_hip_timer_start": (_i, [_vp]),
    "gsl_sinterp_hip_timer_stop": (_i, [_vp, C.POINTER(C.c_float)]),
    "gsl_sinterp_hip_tree_pack": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _pd, _vp]),
    "gsl_sinterp_hip_tree_bind": (_i, [_vp, _i, _vp, _i, _vp, _vp]),
    "gsl_sinterp_hip_bary_eval": (_i, [_vp, _i, _vp, _vp, _pd, _vp, _sz, _sz, _vp, _vp, C.POINTER(C.c_longlong)]),
    "gsl_sinterp_hip_tree_check": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _pd, _i, C.POINTER(C.c_longlong),
                                        C.POINTER(C.c_longlong), _pi]),
    "gsl_sinterp_hip_rbf_fill": (_i, [_vp, _i, _d, _vp, _sz, _i, _sz, _vp, _sz]),
    "gsl_sinterp_hip_cholesky_decomp1": (_i, [_vp, _sz, _vp, _sz, _pi]),
    "gsl_sinterp_hip_cholesky_svx": (_i, [_vp, _sz, _vp, _sz, _vp]),
    "gsl_sinterp_hip_cholesky_factor_solve": (_i, [_vp, _sz, _vp, _sz, _pi, _vp, _sz, _i]),
    "gsl_sinterp_hip_lu_decomp": (_i, [_vp, _sz, _vp, _sz, _vp, _pi]),
    "gsl_sinterp_hip_lu_svx": (_i, [_vp, _sz, _vp, _sz, _vp, _vp]),
    "gsl_sinterp_hip_cholesky_decomp2": (_i, [_vp, _sz, _vp, _sz, _vp, _pi]),
    "gsl_sinterp_hip_cholesky_svx2": (_i, [_vp, _sz, _vp, _sz, _vp, _vp]),
    "gsl_sinterp_hip_cholesky_rcond": (_i, [_vp, _sz, _vp, _sz, _pd]),
    "gsl_sinterp_hip_lu_refine": (_i, [_vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "gsl_sinterp_hip_pcholesky_decomp": (_i, [_vp, _sz, _vp, _sz, _vp]),
    "gsl_sinterp_hip_pcholesky_svx": (_i, [_vp, _sz, _vp, _sz, _vp, _vp]),
    "gsl_sinterp_hip_pcholesky_decomp2": (_i, [_vp, _sz, _vp, _sz, _vp, _vp]),
    "gsl_sinterp_hip_pcholesky_svx2": (_i, [_vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "gsl_sinterp_hip_pcholesky_rcond": (_i, [_vp, _sz, _vp, _sz, _vp, _pd]),
    "gsl_sinterp_hip_rbf_solve_ex": (_i, [_vp, _i, _d, _vp, _sz, _i, _sz, _vp, _sz, _vp, _i, _pd, _pi]),
    "gsl_sinterp_hip_rbf_eval": (_i, [_vp, _i, _d, _vp, _sz, _i, _sz, _vp, _vp, _sz, _sz, _vp]),
    "gsl_sinterp_hip_rbf_eval_model": (_i, [_vp, _i, _d, _vp, _sz, _i, _sz, _vp, _vp, _sz, _sz, _vp, C.c_uint64]),
    "gsl_sinterp_hip_rbf_eval_grad": (_i, [_vp, _i, _d, _pd, _vp, _sz, _i, _sz, _vp, _vp, _sz, _sz, _vp, _vp, _sz, C.c_uint64]),
    "gsl_sinterp_hip_rbf_eval_fields": (_i, [_vp, _i, _d, _pd, _vp, _sz, _i, _sz, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz, C.c_uint64]),
    "gsl_sinterp_hip_rbf_fields_block": (_i, []),
    "gsl_sinterp_hip_rbf_fields_block_small": (_i, []),
    "gsl_sinterp_hip_rbf_solve_fields": (_i, [_vp, _i, _d, _vp, _sz, _i, _sz, _vp, _sz, _vp, _sz, _sz, _pi]),
    "gsl_sinterp_hip_krige_solve_fields": (_i, [_vp, _i, _d, _d, _vp, _sz, _i, _sz, _vp, _sz, _vp, _sz, _sz, _pd, _pi]),
    "gsl_sinterp_hip_ctx_device": (_i, [_vp]),
    "gsl_sinterp_hip_rbf_solve": (_i, [_vp, _i, _d, _vp, _sz, _i, _sz, _vp, _sz, _vp, _pi]),
    "gsl_sinterp_hip_gemm_minus": (_i, [_vp, _sz, _sz, _sz, _vp, _sz, _vp, _sz, _i, _vp, _sz, _i]),
    "gsl_sinterp_hip_grid_targets": (_i, [_vp, _d, _d, _sz, _d, _d, _sz, _vp]),
    "gsl_sinterp_hip_synth_unit": (_i, [_vp, C.c_uint64, C.c_uint64, _d, _d, _vp, _sz]),
    # device groups (multi-GPU target shards)
    "gsl_sinterp_hip_group_create": (_i, [C.POINTER(_vp), _pi, _i]),
    "gsl_sinterp_hip_group_destroy": (None, [_vp]),
    "gsl_sinterp_hip_group_size": (_i, [_vp]),
    "gsl_sinterp_hip_group_device": (_i, [_vp, _i]),
    "gsl_sinterp_hip_group_ctx": (_vp, [_vp, _i]),
    "gsl_sinterp_hip_group_transport": (C.c_char_p, [_vp]),
    "gsl_sinterp_hip_group_last_error": (C.c_char_p, [_vp]),
    "gsl_sinterp_hip_group_broadcast": (_i, [_vp, C.POINTER(_vp), _sz]),
    "gsl_sinterp_hip_shard_bounds": (None, [_sz, _i, _i, C.POINTER(_sz), C.POINTER(_sz)]),
    "gsl_sinterp_hip_h2d_async": (_i, [_vp, _vp, _vp, _sz]),
    "gsl_sinterp_hip_d2h_async": (_i, [_vp, _vp, _vp, _sz]),
    "gsl_sinterp_hip_host_alloc": (_i, [C.POINTER(_vp), _sz]),
    "gsl_sinterp_hip_host_free": (None, [_vp]),
    # --- include/gsl_sinterp.h part 1 (reference symbols)
    "simplex_tree_node_alloc": (_i, [_pt]),
    "simplex_tree_alloc": (_pt, [_i, _i]),
    "simplex_tree_init": (_i, [_pt, _pm, _pv, _pv, _i, _vp]),
    "simplex_tree_free": (None, [_pt]),
    "simplex_tree_accel_alloc": (_vp, [_i]),
    "simplex_tree_accel_free": (None, [_vp]),
    "point_in_simplex": (_i, [_pt, _i, _i]),
    "find_leaf": (_i, [_pt, _pm, _pv, _vp]),
    "_find_leaf": (_i, [_pt, _i, _pm, _pv, _vp]),
    "insert_point": (_i, [_pt, _i, _pm, _pv, _vp]),
    "in_hypersphere": (_i, [_pt, _i, _pm, _i, _vp]),
    "in_hypersphere_points": (_i, [_pt, _pi, _pm, _i, _vp]),
    "calculate_hypersphere": (_i, [_pt, _i, _pm, _pv, _pd, _vp]),
    "calculate_hypersphere_points": (_i, [_pt, _pi, _pm, _pv, _pd, _vp]),
    "calculate_bary_coords": (_i, [_pt, _i, _pm, _pv, _vp]),
    "contains_point": (_i, [_pt, _i, _pm, _pv, _vp]),
    "interp_point": (_d, [_pt, _i, _pm, _pv, _pv, _vp]),
    "delaunay": (_i, [_pt, _i, _pm, _i, _vp]),
    # --- part 2
    "simplex_tree_device_alloc": (_vp, [_pt, _pm, _i]),
    "simplex_tree_device_free": (None, [_vp]),
    "simplex_tree_device_set_response": (_i, [_vp, _pv]),
    "simplex_tree_device_eval_many": (_i, [_vp, _pm, _pv, _pi]),
    "simplex_tree_device_eval_resident": (_i, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "simplex_tree_device_ctx": (_vp, [_vp]),
    "simplex_tree_device_set_responses": (_i, [_vp, _pm]),
    "simplex_tree_device_n_responses": (_sz, [_vp]),
    "simplex_tree_device_eval_fields_many": (_i, [_vp, _pm, _pm, _pm, _pi]),
    "simplex_tree_device_eval_fields_resident": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _vp]),
    "check_leaf_nodes": (None, [_pt, _vp]),
    "check_delaunay": (_i, [_pt, _pm]),
    "output_triangulation": (None, [_pt, _pm, _pv, _i, C.c_char_p, C.c_char_p, C.c_char_p]),
    "simplex_tree_fwrite": (_i, [_vp, _pt]),
    "simplex_tree_fread": (_pt, [_vp]),
    "simplex_tree_check_device": (_i, [_pt, _pm, _i, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "simplex_tree_device_alloc_multi": (_vp, [_pt, _pm, _pi, _i]),
    "simplex_tree_device_n_devices": (_i, [_vp]),
    "simplex_tree_device_transport": (C.c_char_p, [_vp]),
    # --- part 2b: imported triangulations
    "simplex_mesh_import": (_vp, [_pm, _pi, _pi, _sz]),
    "simplex_mesh_import_nd": (_vp, [_pm, _sz, _pi, _pi, _sz]),
    "simplex_mesh_dim": (_sz, [_vp]),
    "simplex_mesh_from_tree": (_vp, [_pt, _pm]),
    "simplex_mesh_free": (None, [_vp]),
    "simplex_mesh_n_triangles": (_sz, [_vp]),
    "simplex_mesh_n_points": (_sz, [_vp]),
    "simplex_mesh_triangles": (_pi, [_vp]),
    "simplex_mesh_neighbours": (_pi, [_vp]),
    "simplex_mesh_tree_nodes": (_pi, [_vp]),
    "simplex_mesh_geometry": (None, [_vp, _pd, _pd]),
    "simplex_mesh_bbox": (None, [_vp, _pd, _pd]),
    "simplex_mesh_points": (_pd, [_vp]),
    "simplex_mesh_set_convex": (None, [_vp, _i]),
    "simplex_mesh_convex": (_i, [_vp]),
    "simplex_mesh_delaunay_metric": (_i, [_vp]),
    "simplex_mesh_vertex_adjacency": (_i, [_vp, _pi, _pi, _sz, C.POINTER(_sz)]),
    "simplex_mesh_device_alloc": (_vp, [_vp, _i]),
    "simplex_mesh_device_alloc_multi": (_vp, [_vp, _pi, _i]),
    "simplex_mesh_device_n_devices": (_i, [_vp]),
    "simplex_mesh_fwrite": (_i, [_vp, _vp]),
    "simplex_mesh_fread": (_vp, [_vp]),
    "gsl_sinterp_set_triangulation": (_i, [C.POINTER(gsl_sinterp), _pi, _pi, _sz]),
    "simplex_mesh_device_free": (None, [_vp]),
    "simplex_mesh_device_set_response": (_i, [_vp, _pv]),
    "simplex_mesh_device_eval_many": (_i, [_vp, _pm, _pv, _pi]),
    "simplex_mesh_device_eval_resident": (_i, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "simplex_mesh_device_ctx": (_vp, [_vp]),
    "simplex_mesh_device_set_responses": (_i, [_vp, _pm]),
    "simplex_mesh_device_n_responses": (_sz, [_vp]),
    "simplex_mesh_device_eval_fields_many": (_i, [_vp, _pm, _pm, _pm, _pi]),
    "simplex_mesh_device_eval_fields_resident": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _vp]),
    "gsl_sinterp_hip_bary_fields_eval": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _sz, _pd, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz]),
    "gsl_sinterp_hip_mesh3_fields_eval": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _sz, _pd, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz]),
    "gsl_sinterp_hip_sort_wanted": (_i, [_sz]),
    "simplex_mesh_device_eval_natural_many": (_i, [_vp, _pm, _pv, _pi]),
    "simplex_mesh_device_eval_natural_resident": (_i, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "simplex_mesh_device_bind_gradients": (_i, [_vp, _pm]),
    "simplex_mesh_device_set_gradient_options": (_i, [_vp, _d, _sz]),
    "simplex_mesh_device_gradients": (_i, [_vp, _pm, C.POINTER(_sz), _pd]),
    "simplex_mesh_device_eval_cubic_many": (_i, [_vp, _pm, _pv, _pm, _pi]),
    "simplex_mesh_device_eval_cubic_resident": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp]),
    "gsl_sinterp_hip_mesh_cubic_gradients": (_i, [_vp, _i, _vp, _vp, _sz, _vp, _vp, _d, _i, _vp, _pi, _pd]),
    "gsl_sinterp_hip_mesh_cubic_pack": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "gsl_sinterp_hip_mesh_cubic_eval": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz]),
    "gsl_sinterp_hip_mesh_natural_pack": (_i, [_vp, _i, _vp, _vp, _i, _vp, _pd, _vp]),
    "gsl_sinterp_hip_mesh_natural_eval": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _i, _vp, C.POINTER(C.c_longlong)]),
    "gsl_sinterp_hip_mesh_pack": (_i, [_vp, _i, _vp, _vp, _i, _vp, _pd, _i, _vp, _vp]),
    "gsl_sinterp_hip_mesh_eval": (_i, [_vp, _i, _vp, _vp, _vp, _i, _pd, _i, _vp, _sz, _sz, _vp, _vp, C.POINTER(C.c_longlong)]),
    "gsl_sinterp_hip_mesh3_pack": (_i, [_vp, _i, _vp, _vp, _i, _vp, _pd, _i, _vp, _vp]),
    "gsl_sinterp_hip_mesh3_bind": (_i, [_vp, _i, _vp, _i, _vp, _vp]),
    "gsl_sinterp_hip_mesh3_eval": (_i, [_vp, _i, _vp, _vp, _vp, _i, _pd, _i, _vp, _sz, _sz, _vp, _vp, C.POINTER(C.c_longlong)]),
    # --- part 3
    "gsl_sinterp_alloc": (C.POINTER(gsl_sinterp), [_vp, _sz, _sz]),
    "gsl_sinterp_set_device": (_i, [C.POINTER(gsl_sinterp), _i]),
    "gsl_sinterp_set_shape": (_i, [C.POINTER(gsl_sinterp), _d]),
    "gsl_sinterp_set_solver": (_i, [C.POINTER(gsl_sinterp), _i]),
    "gsl_sinterp_set_nugget": (_i, [C.POINTER(gsl_sinterp), _d]),
    "gsl_sinterp_mean": (_i, [C.POINTER(gsl_sinterp), _pd]),
    "gsl_sinterp_poly": (_i, [C.POINTER(gsl_sinterp), _pv]),
    "gsl_sinterp_hip_pipe_create": (_i, [_vp, C.POINTER(_vp)]),
    "gsl_sinterp_hip_pipe_destroy": (None, [_vp]),
    "gsl_sinterp_hip_pipe_upload": (_i, [_vp, _vp, _vp, _sz]),
    "gsl_sinterp_hip_pipe_mark": (_i, [_vp, _pi]),
    "gsl_sinterp_hip_pipe_download": (_i, [_vp, _i, _vp, _vp, _sz]),
    "gsl_sinterp_hip_pipe_sync": (_i, [_vp]),
    "gsl_sinterp_hip_bary_last_queue": (_i, [_vp, C.POINTER(C.c_uint), _pi]),
    "gsl_sinterp_hip_count_negative": (_i, [_vp, _vp, _sz, C.POINTER(C.c_longlong)]),
    "gsl_sinterp_hip_rbf_solve_affine": (_i, [_vp, _i, _d, _vp, _sz, _i, _sz, _vp, _sz, _vp, _pd, _pi]),
    "gsl_sinterp_hip_rbf_eval_affine": (_i, [_vp, _i, _d, _pd, _vp, _sz, _i, _sz, _vp, _vp, _sz, _sz, _vp, C.c_uint64]),
    "gsl_sinterp_hip_krige_solve": (_i, [_vp, _i, _d, _d, _vp, _sz, _i, _sz, _vp, _sz, _vp, _pd, _pi]),
    "gsl_sinterp_hip_krige_eval": (_i, [_vp, _i, _d, _d, _vp, _sz, _i, _sz, _vp, _vp, _sz, _sz, _vp, C.c_uint64]),
    "gsl_sinterp_hip_krige_variance_prepare": (_i, [_vp, _sz, _vp, _sz, _vp, _vp, _pd]),
    "gsl_sinterp_hip_krige_variance_work": (_sz, [_sz, _sz]),
    "gsl_sinterp_hip_krige_variance": (_i, [_vp, _i, _d, _vp, _sz, _i, _sz, _vp, _sz, _vp, _vp, _d, _vp, _sz, _sz, _vp, _vp, _sz]),
    "gsl_sinterp_hip_krige_variance_clamp": (_i, [_vp, _vp, _sz]),
    "gsl_sinterp_set_variance": (_i, [C.POINTER(gsl_sinterp), _i]),
    "gsl_sinterp_eval_variance_e": (_i, [C.POINTER(gsl_sinterp), _pv, _pd]),
    "gsl_sinterp_eval_variance_many": (_i, [C.POINTER(gsl_sinterp), _pm, _pv]),
    "gsl_sinterp_eval_variance_resident": (_i, [C.POINTER(gsl_sinterp), _vp, _sz, _sz, _vp]),
    "gsl_sinterp_hip_chol_inv_diag_work": (_sz, [_sz, _sz]),
    "gsl_sinterp_hip_chol_inv_diag": (_i, [_vp, _sz, _vp, _sz, _vp, _vp, _sz]),
    "gsl_sinterp_hip_loo_combine": (_i, [_vp, _sz, _sz, _vp, _vp, _d, _vp, _sz, _vp, _sz, _vp]),
    "gsl_sinterp_hip_drift_terms": (_sz, [_i, _i]),
    "gsl_sinterp_hip_drift_factor": (_i, [_sz, _pd, _pd]),
    "gsl_sinterp_hip_drift_basis": (_i, [_vp, _i, _pd, _pd, _vp, _sz, _i, _sz, _vp, _sz]),
    "gsl_sinterp_hip_ukrige_solve": (_i, [_vp, _i, _d, _d, _i, _pd, _pd, _vp, _sz, _i, _sz, _vp, _sz, _vp, _sz, _sz, _pd, _vp, _sz, _pd, _pd, _vp,
                                          _pi]),
    "gsl_sinterp_hip_drift_add": (_i, [_vp, _i, _pd, _pd, _pd, _sz, _vp, _sz, _i, _sz, _vp, _sz, _vp, _sz]),
    "gsl_sinterp_hip_ukrige_variance_work": (_sz, [_sz, _sz, _sz]),
    "gsl_sinterp_hip_ukrige_variance": (_i, [_vp, _i, _d, _i, _pd, _pd, _vp, _sz, _i, _sz, _vp, _sz, _vp, _sz, _vp, _pd, _vp, _sz, _sz, _vp,
                                             _vp, _sz]),
    "gsl_sinterp_hip_loo_combine_drift": (_i, [_vp, _sz, _sz, _vp, _vp, _sz, _sz, _pd, _vp, _sz, _vp, _sz, _vp]),
    "gsl_sinterp_hip_krige_covariance_work": (_sz, [_sz, _sz, _sz, _sz]),
    "gsl_sinterp_hip_krige_covariance": (_i, [_vp, _i, _d, _i, _pd, _pd, _vp, _sz, _i, _sz, _vp, _sz, _vp, _sz, _vp, _pd, _vp, _sz, _sz, _vp,
                                              _sz, _sz, _vp, _sz, _vp]),
    "gsl_sinterp_hip_krige_simulate_work": (_sz, [_sz, _sz, _sz, _sz]),
    "gsl_sinterp_hip_krige_simulate": (_i, [_vp, _i, _d, _i, _pd, _pd, _vp, _sz, _i, _sz, _vp, _sz, _vp, _sz, _vp, _pd, _vp, _sz, _sz, _vp,
                                            _d, _d, _vp, _sz, _sz, _vp, _sz, _vp]),
    "gsl_sinterp_eval_covariance_many": (_i, [C.POINTER(gsl_sinterp), _pm, _pm, _pm]),
    "gsl_sinterp_eval_covariance_resident": (_i, [C.POINTER(gsl_sinterp), _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz]),
    "gsl_sinterp_simulate_many": (_i, [C.POINTER(gsl_sinterp), _pm, _d, _d, _pm, _pm]),
    "gsl_sinterp_simulate_resident": (_i, [C.POINTER(gsl_sinterp), _vp, _sz, _sz, _d, _d, _vp, _sz, _sz, _vp, _sz]),
    "gsl_sinterp_set_drift": (_i, [C.POINTER(gsl_sinterp), _i]),
    "gsl_sinterp_drift": (_i, [C.POINTER(gsl_sinterp)]),
    "gsl_sinterp_drift_terms": (_sz, [_sz, _i]),
    "gsl_sinterp_drift_coefficients": (_i, [C.POINTER(gsl_sinterp), _sz, _pv, _pv, _pv]),
    "gsl_sinterp_set_loo": (_i, [C.POINTER(gsl_sinterp), _i]),
    "gsl_sinterp_loo_residuals": (_i, [C.POINTER(gsl_sinterp), _pm]),
    "gsl_sinterp_loo_variance": (_i, [C.POINTER(gsl_sinterp), _pv]),
    "gsl_sinterp_hip_d2d_async": (_i, [_vp, _vp, _vp, _sz]),
    "gsl_sinterp_hip_knn": (_i, [_vp, _vp, _sz, _i, _sz, _vp, _sz, _sz, _sz, _vp, _vp, C.c_uint64]),
    "gsl_sinterp_hip_local_krige": (_i, [_vp, _i, _d, _d, _vp, _sz, _i, _sz, _vp, _vp, _sz, _sz, _sz, _vp, _vp, _vp,
                                         C.POINTER(C.c_size_t), C.c_uint64]),
    "gsl_sinterp_hip_local_ukrige": (_i, [_vp, _i, _d, _d, _vp, _sz, _i, _sz, _vp, _vp, _sz, _sz, _sz, _vp, _vp, _vp,
                                          C.POINTER(C.c_size_t), C.c_uint64]),
    "gsl_sinterp_hip_local_pack": (_i, [_vp, _vp, _sz, _i, _sz, _vp, C.c_uint64]),
    "gsl_sinterp_hip_local_pack_count": (C.c_uint64, [_vp]),
    "gsl_sinterp_set_neighbours": (_i, [C.POINTER(gsl_sinterp), _sz]),
    "gsl_sinterp_hip_shepard_fit": (_i, [_vp, _vp, _sz, _i, _sz, _vp, _sz, _sz, _vp, _vp, _vp, C.POINTER(C.c_size_t)]),
    "gsl_sinterp_hip_shepard_eval": (_i, [_vp, _vp, _sz, _i, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp,
                                          C.POINTER(C.c_size_t), C.c_uint64]),
    "gsl_sinterp_hip_shepard_pack_count": (C.c_uint64, [_vp]),
    "gsl_sinterp_hip_shepard_fit_count": (C.c_uint64, [_vp]),
    "gsl_sinterp_set_shepard": (_i, [C.POINTER(gsl_sinterp), _sz, _sz]),
    "gsl_sinterp_shepard_stats": (_i, [C.POINTER(gsl_sinterp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _pd]),
    "gsl_sinterp_shepard_ctx": (_vp, [C.POINTER(gsl_sinterp)]),
    "gsl_sinterp_eval_local_many": (_i, [C.POINTER(gsl_sinterp), _pm, _pv, _pv, _pi]),
    "gsl_sinterp_hip_score_reduce": (_i, [_vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _d, _vp]),
    "gsl_sinterp_fit_alloc": (_vp, [C.POINTER(gsl_sinterp), _pm, _pv]),
    "gsl_sinterp_fit_free": (None, [_vp]),
    "gsl_sinterp_fit_score": (_i, [_vp, _i, _d, _d, _pd]),
    "gsl_sinterp_fit_shape": (_i, [_vp, _i, _d, _d, _d, _pd, _pd]),
    "gsl_sinterp_fit_nugget": (_i, [_vp, _i, _d, _d, _d, _pd, _pd]),
    "gsl_sinterp_fit_set_search": (_i, [_vp, _sz, _d, _sz]),
    "gsl_sinterp_fit_n_eval": (_sz, [_vp]),
    "gsl_sinterp_fit_trace": (_i, [_vp, _pv, _pv]),
    "gsl_sinterp_fit_sigma2": (_i, [_vp, _pd]),
    "gsl_sinterp_hip_variogram": (_i, [_vp, _vp, _sz, _i, _sz, _vp, _d, _i, C.POINTER(C.c_uint64), _pi]),
    "gsl_sinterp_hip_variogram_pairs_tested": (C.c_uint64, [_vp]),
    "gsl_sinterp_hip_bbox": (_i, [_vp, _vp, _sz, _i, _sz, _pd]),
    "gsl_sinterp_variogram_alloc": (_vp, [_sz, _sz]),
    "gsl_sinterp_variogram_set_device": (_i, [_vp, _i]),
    "gsl_sinterp_variogram_compute": (_i, [_vp, _pm, _pv, _d]),
    "gsl_sinterp_variogram_compute_resident": (_i, [_vp, _vp, _sz, _sz, _vp, _d]),
    "gsl_sinterp_variogram_get": (_i, [_vp, _i, _pv, _pv, _pv]),
    "gsl_sinterp_variogram_h_max": (_d, [_vp]),
    "gsl_sinterp_variogram_fit": (_i, [_vp, _vp, _i, _i, _d, _d, _pd, _pd, _pd, _pd]),
    "gsl_sinterp_variogram_apply": (_i, [_vp, C.POINTER(gsl_sinterp)]),
    "gsl_sinterp_variogram_free": (None, [_vp]),
    "gsl_sinterp_variogram_fit_model": (_i, [_i, _i, _pd, _pd, _pd, _sz, _d, _d, _sz, _d, _sz, _pd, _pd, _pd, _pd]),
    "gsl_sinterp_variogram_fit_model_n_eval": (_sz, []),
    "gsl_sinterp_variogram_fit_model_trace": (_i, [_pv, _pv]),
    "gsl_sinterp_eval_grad_e": (_i, [C.POINTER(gsl_sinterp), _pv, _pd, _pv]),
    "gsl_sinterp_eval_grad_many": (_i, [C.POINTER(gsl_sinterp), _pm, _pv, _pm]),
    "gsl_sinterp_eval_grad_resident": (_i, [C.POINTER(gsl_sinterp), _vp, _sz, _sz, _vp, _vp, _sz]),
    "gsl_sinterp_init_fields": (_i, [C.POINTER(gsl_sinterp), _pm, _pm]),
    "gsl_sinterp_n_fields": (_sz, [C.POINTER(gsl_sinterp)]),
    "gsl_sinterp_eval_fields_e": (_i, [C.POINTER(gsl_sinterp), _pv, _pv]),
    "gsl_sinterp_eval_fields_many": (_i, [C.POINTER(gsl_sinterp), _pm, _pm]),
    "gsl_sinterp_eval_fields_resident": (_i, [C.POINTER(gsl_sinterp), _vp, _sz, _sz, _vp, _sz]),
    "gsl_sinterp_linear_init_fields": (_i, [C.POINTER(gsl_sinterp), _pm, _pm]),
    "gsl_sinterp_linear_eval_fields_e": (_i, [C.POINTER(gsl_sinterp), _pv, _pv, _pm]),
    "gsl_sinterp_linear_eval_fields_many": (_i, [C.POINTER(gsl_sinterp), _pm, _pm, _pm, _pi]),
    "gsl_sinterp_linear_eval_fields_resident": (_i, [C.POINTER(gsl_sinterp), _vp, _sz, _sz, _vp, _sz, _vp, _sz, _vp]),
    "gsl_sinterp_get_field_weights": (_i, [C.POINTER(gsl_sinterp), _sz, _pv]),
    "gsl_sinterp_field_mean": (_i, [C.POINTER(gsl_sinterp), _sz, _pd]),
    "gsl_sinterp_field_poly": (_i, [C.POINTER(gsl_sinterp), _sz, _pv]),
    "gsl_sinterp_set_rcond": (_i, [C.POINTER(gsl_sinterp), _i]),
    "gsl_sinterp_rcond": (_i, [C.POINTER(gsl_sinterp), _pd]),
    "gsl_sinterp_route": (_i, [C.POINTER(gsl_sinterp)]),
    "gsl_sinterp_set_devices": (_i, [C.POINTER(gsl_sinterp), _i]),
    "gsl_sinterp_set_device_list": (_i, [C.POINTER(gsl_sinterp), _pi, _i]),
    "gsl_sinterp_n_devices": (_i, [C.POINTER(gsl_sinterp)]),
    "gsl_sinterp_set_tree_options": (_i, [C.POINTER(gsl_sinterp), _i, _vp]),
    "gsl_sinterp_set_gradients": (_i, [C.POINTER(gsl_sinterp), _pm]),
    "gsl_sinterp_set_gradient_options": (_i, [C.POINTER(gsl_sinterp), _d, _sz]),
    "gsl_sinterp_get_gradients": (_i, [C.POINTER(gsl_sinterp), _pm, C.POINTER(_sz), _pd]),
    "gsl_sinterp_init": (_i, [C.POINTER(gsl_sinterp), _pm, _pv]),
    "gsl_sinterp_name": (C.c_char_p, [C.POINTER(gsl_sinterp)]),
    "gsl_sinterp_min_size": (C.c_uint, [C.POINTER(gsl_sinterp)]),
    "gsl_sinterp_eval_e": (_i, [C.POINTER(gsl_sinterp), _pv, _pd]),
    "gsl_sinterp_eval": (_d, [C.POINTER(gsl_sinterp), _pv]),
    "gsl_sinterp_eval_many": (_i, [C.POINTER(gsl_sinterp), _pm, _pv, _pi]),
    "gsl_sinterp_eval_resident": (_i, [C.POINTER(gsl_sinterp), _vp, _sz, _sz, _vp, _vp]),
    "gsl_sinterp_eval_grid": (_i, [C.POINTER(gsl_sinterp), _pv, _pv, _pm]),
    "gsl_sinterp_fprintf_grid": (_i, [_vp, _pv, _pv, _pm]),
    "gsl_sinterp_fwrite": (_i, [_vp, C.POINTER(gsl_sinterp)]),
    "gsl_sinterp_fread": (_i, [_vp, C.POINTER(gsl_sinterp)]),
    "gsl_sinterp_get_weights": (_i, [C.POINTER(gsl_sinterp), _pv]),
    "gsl_sinterp_free": (None, [C.POINTER(gsl_sinterp)]),
    # --- compat slice used by the bindings
    "gsl_set_error_handler_off": (_vp, []),
    "gsl_set_error_handler": (_vp, [_vp]),
    "gsl_rng_alloc": (_vp, [_vp]),
    "gsl_rng_set": (None, [_vp, C.c_ulong]),
    "gsl_rng_free": (None, [_vp]),
    "gsl_rng_get": (C.c_ulong, [_vp]),
    "gsl_rng_uniform_int": (C.c_ulong, [_vp, C.c_ulong]),
}
DATA_SYMBOLS = ["gsl_sinterp_kriging", "gsl_sinterp_linear_mesh", "gsl_sinterp_natural_mesh", "gsl_sinterp_natural_simplex", "gsl_sinterp_cubic_mesh", "gsl_sinterp_cubic_simplex", "gsl_sinterp_shepard", "gsl_sinterp_rbf_gaussian", "gsl_sinterp_rbf_tps", "gsl_sinterp_rbf_tps_affine", "gsl_sinterp_rbf_wendland", "gsl_sinterp_linear_simplex",
                "gsl_sinterp_rbf_matern32", "gsl_sinterp_rbf_matern52", "gsl_sinterp_rbf_imq", "gsl_sinterp_kriging_matern32", "gsl_sinterp_kriging_matern52",
                "gsl_rng_mt19937", "gsl_rng_default"]


def _declare(L):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args


def _ptr(symbol):
    """value of an exported `const T *symbol` variable"""
    return C.c_void_p.in_dll(lib(), symbol).value


# ------------------------------------------------------------------ C stdio (FILE * arguments)
_libc = C.CDLL(None)
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]


class CFile:
    """`with CFile(path, "wb") as fp:` -> a FILE * for the library's fwrite / fread / fprintf entries."""

    def __init__(self, path, mode):
        self.fp = _libc.fopen(str(path).encode(), mode.encode())
        if not self.fp:
            raise OSError(f"fopen({path!r}, {mode!r}) failed")

    def __enter__(self):
        return C.c_void_p(self.fp)

    def __exit__(self, *exc):
        _libc.fclose(C.c_void_p(self.fp))
        self.fp = None


# ------------------------------------------------------------------ views
def as_matrix(a):
    """gsl_matrix view of a 2-D float64 numpy array (row stride honoured)."""
    assert a.dtype == np.float64 and a.ndim == 2 and (a.size == 0 or a.strides[1] == 8)
    m = gsl_matrix()
    m.size1, m.size2 = a.shape[0], a.shape[1]
    m.tda = a.strides[0] // 8 if a.shape[0] > 1 and a.size else max(a.shape[1], 1)
    m.data = a.ctypes.data_as(_pd)
    m.block, m.owner = None, 0
    m._keep = a
    return m


def as_vector(a):
    assert a.dtype == np.float64 and a.ndim == 1
    v = gsl_vector()
    v.size, v.stride = a.shape[0], (a.strides[0] // 8 if a.shape[0] > 1 else 1)
    v.data = a.ctypes.data_as(_pd)
    v.block, v.owner = None, 0
    v._keep = a
    return v


class GslError(RuntimeError):
    def __init__(self, status, what=""):
        super().__init__(f"GSL status {status} {what}")
        self.status = status


class ErrorCalls:
    """`with ErrorCalls() as calls:` -- the (reason, status) of every call the library makes to the GSL error handler inside
    the block (the bindings otherwise keep the handler off); the previous handler is restored on exit.  How an entry that
    returns a pointer reports its status, and how a test sees that the handler was NOT called."""
    _TYPE = C.CFUNCTYPE(None, C.c_char_p, C.c_char_p, C.c_int, C.c_int)

    def __enter__(self):
        self.calls = []
        self._cb = self._TYPE(lambda reason, file, line, status: self.calls.append(((reason or b"").decode(), status)))
        self._prev = lib().gsl_set_error_handler(C.cast(self._cb, C.c_void_p))
        return self.calls

    def __exit__(self, *exc):
        lib().gsl_set_error_handler(self._prev)


def check(status, ctx=None):
    if status != GSL_SUCCESS:
        msg = lib().gsl_sinterp_hip_last_error(ctx).decode() if ctx else ""
        raise GslError(status, msg)


# ------------------------------------------------------------------ HIP context
class HipContext:
    """gsl_sinterp_hip_ctx bound to one device and (optionally) torch's current stream."""

    def __init__(self, device=0, stream=None):
        L = lib()
        if L.gsl_sinterp_hip_device_count() <= 0:
            raise RuntimeError("no HIP device visible: the gfx950 kernels cannot run (no CPU fallback exists)")
        self._h = C.c_void_p()
        st = L.gsl_sinterp_hip_ctx_create(C.byref(self._h), device, stream)
        if st != GSL_SUCCESS:
            raise GslError(st, "gsl_sinterp_hip_ctx_create")
        self.device = device

    @classmethod
    def on_torch_stream(cls, device=0):
        import torch
        torch.cuda.set_device(device)
        return cls(device, C.c_void_p(torch.cuda.current_stream(device).cuda_stream))

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().gsl_sinterp_hip_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(lib().gsl_sinterp_hip_sync(self._h), self._h)

    # thin wrappers: every pointer argument is an int device address
    def tree_pack(self, n_nodes, d_type, d_pidx, d_links, n_points, d_points, geom, d_records):
        g = np.ascontiguousarray(geom, dtype=np.float64)
        check(lib().gsl_sinterp_hip_tree_pack(self._h, n_nodes, d_type, d_pidx, d_links, n_points, d_points,
                                              g.ctypes.data_as(_pd), d_records), self._h)

    def tree_bind(self, n_nodes, d_pidx, n_points, d_response, d_leaftab):
        check(lib().gsl_sinterp_hip_tree_bind(self._h, n_nodes, d_pidx, n_points, d_response, d_leaftab), self._h)

    def mesh_natural_pack(self, n_tri, d_tri, d_nbr, n_points, d_points, metric, d_nnrec):
        """natural-neighbour records: (n_tri + 1) * NATURAL_RECORD_BYTES bytes at d_nnrec; metric = the per-axis factors"""
        g = np.ascontiguousarray(metric, dtype=np.float64)
        check(lib().gsl_sinterp_hip_mesh_natural_pack(self._h, n_tri, d_tri, d_nbr, n_points, d_points, g.ctypes.data_as(_pd), d_nnrec),
              self._h)

    def mesh_natural_eval(self, n_tri, d_nnrec, d_leaftab, d_located, d_linear_values, d_targets, m, ttda, d_values, depth_cap=0):
        """the cavity sweep over the triangles gsl_sinterp_hip_mesh_eval located; returns how many targets took the scan"""
        cnt = C.c_longlong(0)
        check(lib().gsl_sinterp_hip_mesh_natural_eval(self._h, n_tri, d_nnrec, d_leaftab, d_located, d_linear_values, d_targets, m, ttda,
                                                      depth_cap, d_values, C.byref(cnt)), self._h)
        return cnt.value

    def mesh_cubic_gradients(self, n_points, d_offsets, d_adjacent, n_adjacent, d_points, d_f, d_g, rtol=1e-12, maxiter=1000):
        """(status, iterations, residual): the Clough-Tocher vertex gradients into d_g [2 n_points]; GSL_EMAXITER is returned, not raised"""
        it, res = C.c_int(0), C.c_double(0.0)
        st = lib().gsl_sinterp_hip_mesh_cubic_gradients(self._h, n_points, d_offsets, d_adjacent, n_adjacent, d_points, d_f, rtol, maxiter,
                                                        d_g, C.byref(it), C.byref(res))
        if st != GSL_EMAXITER:
            check(st, self._h)
        return st, it.value, res.value

    def mesh_cubic_pack(self, n_tri, d_tri, d_nbr, n_points, d_points, d_f, d_g, d_ctrec):
        """Clough-Tocher records: n_tri * CUBIC_RECORD_BYTES bytes at d_ctrec"""
        check(lib().gsl_sinterp_hip_mesh_cubic_pack(self._h, n_tri, d_tri, d_nbr, n_points, d_points, d_f, d_g, d_ctrec), self._h)

    def mesh_cubic_eval(self, n_tri, d_ctrec, d_located, d_linear_values, d_targets, m, ttda, d_values, d_grad=None, gtda=2):
        """the cubic sweep over the triangles gsl_sinterp_hip_mesh_eval located; d_grad = None: values only"""
        check(lib().gsl_sinterp_hip_mesh_cubic_eval(self._h, n_tri, d_ctrec, d_located, d_linear_values, d_targets, m, ttda, d_values,
                                                    d_grad, gtda), self._h)

    def bary_eval(self, n_nodes, d_records, d_leaftab, scale, d_targets, m, ttda, d_values, d_leaf=None,
                  count_outside=False):
        s = np.ascontiguousarray(scale, dtype=np.float64)
        cnt = C.c_longlong(0)
        st = lib().gsl_sinterp_hip_bary_eval(self._h, n_nodes, d_records, d_leaftab, s.ctypes.data_as(_pd), d_targets,
                                             m, ttda, d_values, d_leaf, C.byref(cnt) if count_outside else None)
        if st not in (GSL_SUCCESS, GSL_EDOM):
            check(st, self._h)
        return cnt.value

    def rbf_fill(self, kind, eps, d_x, n, dim, xtda, d_phi, lda):
        check(lib().gsl_sinterp_hip_rbf_fill(self._h, kind, eps, d_x, n, dim, xtda, d_phi, lda), self._h)

    def cholesky_decomp1(self, n, d_a, lda):
        info = C.c_int(0)
        st = lib().gsl_sinterp_hip_cholesky_decomp1(self._h, n, d_a, lda, C.byref(info))
        return st, info.value

    def cholesky_svx(self, n, d_llt, lda, d_x):
        check(lib().gsl_sinterp_hip_cholesky_svx(self._h, n, d_llt, lda, d_x), self._h)

    def cholesky_factor_solve(self, n, d_a, lda, d_x, ldx, nrhs):
        """cholesky_decomp1 + the solve of nrhs columns d_x + q*ldx in place; returns (status, info)"""
        info = C.c_int(0)
        st = lib().gsl_sinterp_hip_cholesky_factor_solve(self._h, n, d_a, lda, C.byref(info), d_x, ldx, nrhs)
        return st, info.value

    def lu_decomp(self, n, d_a, lda, d_perm):
        sg = C.c_int(0)
        check(lib().gsl_sinterp_hip_lu_decomp(self._h, n, d_a, lda, d_perm, C.byref(sg)), self._h)
        return sg.value

    def lu_svx(self, n, d_lu, lda, d_perm, d_x):
        return lib().gsl_sinterp_hip_lu_svx(self._h, n, d_lu, lda, d_perm, d_x)

    def rbf_eval(self, kind, eps, d_x, n, dim, xtda, d_w, d_y, m, ytda, d_s, model_id=0):
        """model_id != 0: the caller vouches that (d_x, d_w) do not change while it uses this id, so the sweep's
        per-model preprocessing is cached in the context (gsl_sinterp_hip_rbf_eval_model)"""
        check(lib().gsl_sinterp_hip_rbf_eval_model(self._h, kind, eps, d_x, n, dim, xtda, d_w, d_y, m, ytda, d_s, model_id), self._h)

    def rbf_eval_grad(self, kind, eps, d_x, n, dim, xtda, d_w, d_y, m, ytda, d_s, d_g, gtda, tail=None, model_id=0):
        """value (d_s, may be None) + gradient (row k at d_g + 8 k gtda) from one sweep; tail: None or dim + 1 numbers
        {c_0, c_1 .. c_dim} of an affine tail.  Returns the status."""
        t = None if tail is None else np.ascontiguousarray(tail, dtype=np.float64)
        assert t is None or t.size >= dim + 1
        return lib().gsl_sinterp_hip_rbf_eval_grad(self._h, kind, eps, None if t is None else t.ctypes.data_as(_pd), d_x, n, dim, xtda,
                                                   d_w, d_y, m, ytda, d_s, d_g, gtda, model_id)

    def rbf_eval_fields(self, kind, eps, d_x, n, dim, xtda, d_w, ldw, nf, d_y, m, ytda, d_s, stda, tail=None, model_id=0):
        """nf fields from one sweep: column q of the weights at d_w + 8 q ldw, target k's field q at d_s + 8 (k stda + q);
        tail: None or nf x (dim + 1) numbers, {c_0 .. c_dim} per field.  Returns the status."""
        t = None if tail is None else np.ascontiguousarray(tail, dtype=np.float64).reshape(-1)
        assert t is None or t.size >= nf * (dim + 1)
        return lib().gsl_sinterp_hip_rbf_eval_fields(self._h, kind, eps, None if t is None else t.ctypes.data_as(_pd), d_x, n, dim, xtda,
                                                     d_w, ldw, nf, d_y, m, ytda, d_s, stda, model_id)

    @staticmethod
    def rbf_fields_block():
        """fields per pass of the fields sweep (the library's compile-time NF)"""
        return lib().gsl_sinterp_hip_rbf_fields_block()

    @staticmethod
    def rbf_fields_block_small():
        """the last <= this many fields of a sweep go through the small instance"""
        return lib().gsl_sinterp_hip_rbf_fields_block_small()

    def rbf_solve_fields(self, kind, eps, d_x, n, dim, xtda, d_phi, lda, d_w, ldw, nf):
        """one fill, one Cholesky, nf solves in place (column q at d_w + 8 q ldw); returns (status, route)"""
        route = C.c_int(0)
        st = lib().gsl_sinterp_hip_rbf_solve_fields(self._h, kind, eps, d_x, n, dim, xtda, d_phi, lda, d_w, ldw, nf, C.byref(route))
        return st, route.value

    def krige_solve_fields(self, kind, eps, nugget, d_x, n, dim, xtda, d_phi, lda, d_w, ldw, nf):
        """ordinary kriging of nf fields on one factor; returns (status, route, means[nf])"""
        route, mean = C.c_int(0), np.zeros(nf, dtype=np.float64)
        st = lib().gsl_sinterp_hip_krige_solve_fields(self._h, kind, eps, nugget, d_x, n, dim, xtda, d_phi, lda, d_w, ldw, nf,
                                                      mean.ctypes.data_as(_pd), C.byref(route))
        return st, route.value, mean

    # --- universal kriging (csrc/hip/drift.hip): order 1 or 2, h_shift / h_scale = dim doubles each
    @staticmethod
    def drift_terms(dim, order):
        return lib().gsl_sinterp_hip_drift_terms(dim, order)

    @staticmethod
    def drift_factor(S):
        """(status, Ls): the host Cholesky factor of the q x q S, lower triangle, row-major"""
        S = np.ascontiguousarray(S, dtype=np.float64)
        L = np.zeros_like(S)
        st = lib().gsl_sinterp_hip_drift_factor(S.shape[0], S.ctypes.data_as(_pd), L.ctypes.data_as(_pd))
        return st, L

    def drift_basis(self, order, shift, scale, d_x, n, dim, xtda, d_P, ldp):
        shift, scale = np.ascontiguousarray(shift, dtype=np.float64), np.ascontiguousarray(scale, dtype=np.float64)
        return lib().gsl_sinterp_hip_drift_basis(self._h, order, shift.ctypes.data_as(_pd), scale.ctypes.data_as(_pd), d_x, n, dim, xtda,
                                                 d_P, ldp)

    def ukrige_solve(self, kind, eps, nugget, order, shift, scale, d_x, n, dim, xtda, d_phi, lda, d_w, ldw, nf, d_B=None, ldb=0, d_dinv=None):
        """universal kriging of nf fields on one factor; returns (status, route, coef[nf, q], S[q, q], Ls[q, q])"""
        shift, scale = np.ascontiguousarray(shift, dtype=np.float64), np.ascontiguousarray(scale, dtype=np.float64)
        q = max(int(self.drift_terms(dim, order)), 1)
        route, coef, S, Ls = C.c_int(0), np.zeros((max(nf, 1), q)), np.zeros((q, q)), np.zeros((q, q))
        st = lib().gsl_sinterp_hip_ukrige_solve(self._h, kind, eps, nugget, order, shift.ctypes.data_as(_pd), scale.ctypes.data_as(_pd), d_x,
                                                n, dim, xtda, d_phi, lda, d_w, ldw, nf, coef.ctypes.data_as(_pd), d_B, ldb,
                                                S.ctypes.data_as(_pd), Ls.ctypes.data_as(_pd), d_dinv, C.byref(route))
        return st, route.value, coef, S, Ls

    def drift_add(self, order, shift, scale, coef, nf, d_y, m, dim, ytda, d_s, stda, d_g=None, gtda=0):
        """d_s[k stda + f] += p(u(y_k))^T c_f, d_g likewise with the gradient; coef: nf x q"""
        shift, scale = np.ascontiguousarray(shift, dtype=np.float64), np.ascontiguousarray(scale, dtype=np.float64)
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        return lib().gsl_sinterp_hip_drift_add(self._h, order, shift.ctypes.data_as(_pd), scale.ctypes.data_as(_pd), coef.ctypes.data_as(_pd),
                                               nf, d_y, m, dim, ytda, d_s, stda, d_g, gtda)

    @staticmethod
    def ukrige_variance_work(n, chunk, q):
        return lib().gsl_sinterp_hip_ukrige_variance_work(n, chunk, q)

    def ukrige_variance(self, kind, eps, order, shift, scale, d_x, n, dim, xtda, d_llt, lda, d_B, ldb, d_dinv, L, d_y, m, ytda, d_var,
                        d_work, chunk):
        shift, scale = np.ascontiguousarray(shift, dtype=np.float64), np.ascontiguousarray(scale, dtype=np.float64)
        L = np.ascontiguousarray(L, dtype=np.float64)
        return lib().gsl_sinterp_hip_ukrige_variance(self._h, kind, eps, order, shift.ctypes.data_as(_pd), scale.ctypes.data_as(_pd), d_x, n,
                                                     dim, xtda, d_llt, lda, d_B, ldb, d_dinv, L.ctypes.data_as(_pd), d_y, m, ytda, d_var,
                                                     d_work, chunk)

    def loo_combine_drift(self, n, nf, d_g, d_B, ldb, q, L, d_w, ldw, d_e, lde, d_v):
        L = np.ascontiguousarray(L, dtype=np.float64)
        return lib().gsl_sinterp_hip_loo_combine_drift(self._h, n, nf, d_g, d_B, ldb, q, L.ctypes.data_as(_pd), d_w, ldw, d_e, lde, d_v)

    @staticmethod
    def krige_covariance_work(n, ma, mb, q):
        """doubles of d_work that krige_covariance needs (mb = 0: one target set)"""
        return lib().gsl_sinterp_hip_krige_covariance_work(n, ma, mb, q)

    @staticmethod
    def _drift_args(shift, scale, L):
        pd = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        keep = [pd(shift), pd(scale), pd(L)]
        return keep, [None if a is None else a.ctypes.data_as(_pd) for a in keep]

    def krige_covariance(self, kind, eps, order, shift, scale, d_x, n, dim, xtda, d_llt, lda, d_B, ldb, d_dinv, L, d_ya, ma, yatda, d_yb, mb,
                         ybtda, d_cov, ctda, d_work):
        """d_cov = the joint posterior covariance of the targets d_ya x d_yb (d_yb = None: d_ya with itself, symmetric to the bit);
        order 0: shift = scale = None, d_B = b, L = [sqrt(1^T b)]; returns the status"""
        keep, (p_shift, p_scale, p_L) = self._drift_args(shift, scale, L)
        return lib().gsl_sinterp_hip_krige_covariance(self._h, kind, eps, order, p_shift, p_scale, d_x, n, dim, xtda, d_llt, lda, d_B, ldb,
                                                      d_dinv, p_L, d_ya, ma, yatda, d_yb, mb, ybtda, d_cov, ctda, d_work)

    @staticmethod
    def krige_simulate_work(n, m, n_draws, q):
        return lib().gsl_sinterp_hip_krige_simulate_work(n, m, n_draws, q)

    def krige_simulate(self, kind, eps, order, shift, scale, d_x, n, dim, xtda, d_llt, lda, d_B, ldb, d_dinv, L, d_y, m, ytda, d_mean, sigma2,
                       jitter, d_zn, ztda, n_draws, d_out, otda, d_work):
        """d_out = d_mean + sqrt(sigma2) chol(Sigma + jitter I) d_zn; returns the status (GSL_EDOM: not positive definite, NaN)"""
        keep, (p_shift, p_scale, p_L) = self._drift_args(shift, scale, L)
        return lib().gsl_sinterp_hip_krige_simulate(self._h, kind, eps, order, p_shift, p_scale, d_x, n, dim, xtda, d_llt, lda, d_B, ldb, d_dinv,
                                                    p_L, d_y, m, ytda, d_mean, sigma2, jitter, d_zn, ztda, n_draws, d_out, otda, d_work)

    def device(self):
        return lib().gsl_sinterp_hip_ctx_device(self._h)

    def cholesky_decomp2(self, n, d_a, lda, d_s):
        info = C.c_int(0)
        st = lib().gsl_sinterp_hip_cholesky_decomp2(self._h, n, d_a, lda, d_s, C.byref(info))
        return st, info.value

    def cholesky_svx2(self, n, d_llt, lda, d_s, d_x):
        check(lib().gsl_sinterp_hip_cholesky_svx2(self._h, n, d_llt, lda, d_s, d_x), self._h)

    def cholesky_rcond(self, n, d_llt, lda):
        r = C.c_double(0)
        check(lib().gsl_sinterp_hip_cholesky_rcond(self._h, n, d_llt, lda, C.byref(r)), self._h)
        return r.value

    def lu_refine(self, n, d_a, lda, d_lu, ldlu, d_perm, d_b, d_x, d_work):
        return lib().gsl_sinterp_hip_lu_refine(self._h, n, d_a, lda, d_lu, ldlu, d_perm, d_b, d_x, d_work)

    def pcholesky_decomp(self, n, d_a, lda, d_perm):
        check(lib().gsl_sinterp_hip_pcholesky_decomp(self._h, n, d_a, lda, d_perm), self._h)

    def pcholesky_svx(self, n, d_ldlt, lda, d_perm, d_x):
        check(lib().gsl_sinterp_hip_pcholesky_svx(self._h, n, d_ldlt, lda, d_perm, d_x), self._h)

    def pcholesky_decomp2(self, n, d_a, lda, d_perm, d_s):
        check(lib().gsl_sinterp_hip_pcholesky_decomp2(self._h, n, d_a, lda, d_perm, d_s), self._h)

    def pcholesky_svx2(self, n, d_ldlt, lda, d_perm, d_s, d_x):
        check(lib().gsl_sinterp_hip_pcholesky_svx2(self._h, n, d_ldlt, lda, d_perm, d_s, d_x), self._h)

    def pcholesky_rcond(self, n, d_ldlt, lda, d_perm):
        r = C.c_double(0)
        check(lib().gsl_sinterp_hip_pcholesky_rcond(self._h, n, d_ldlt, lda, d_perm, C.byref(r)), self._h)
        return r.value

    def rbf_solve_ex(self, kind, eps, d_x, n, dim, xtda, d_phi, lda, d_w, solver, want_rcond=False):
        route, rc = C.c_int(0), C.c_double(0)
        st = lib().gsl_sinterp_hip_rbf_solve_ex(self._h, kind, eps, d_x, n, dim, xtda, d_phi, lda, d_w, solver,
                                                C.byref(rc) if want_rcond else None, C.byref(route))
        return st, route.value, rc.value

    def rbf_solve(self, kind, eps, d_x, n, dim, xtda, d_phi, lda, d_w):
        route = C.c_int(0)
        st = lib().gsl_sinterp_hip_rbf_solve(self._h, kind, eps, d_x, n, dim, xtda, d_phi, lda, d_w, C.byref(route))
        return st, route.value

    def rbf_solve_affine(self, kind, eps, d_x, n, dim, xtda, d_phi, lda, d_w, h_poly):
        """h_poly: caller's float64 numpy buffer of at least dim + 1 entries (c lands in h_poly[:dim + 1]);
        returns (status, route)"""
        assert h_poly.dtype == np.float64 and h_poly.flags.c_contiguous and h_poly.size >= dim + 1
        route = C.c_int(0)
        st = lib().gsl_sinterp_hip_rbf_solve_affine(self._h, kind, eps, d_x, n, dim, xtda, d_phi, lda, d_w,
                                                    h_poly.ctypes.data_as(_pd), C.byref(route))
        return st, route.value

    def rbf_eval_affine(self, kind, eps, poly, d_x, n, dim, xtda, d_w, d_y, m, ytda, d_s, model_id=0):
        p = np.ascontiguousarray(poly, dtype=np.float64)
        assert p.size >= dim + 1
        check(lib().gsl_sinterp_hip_rbf_eval_affine(self._h, kind, eps, p.ctypes.data_as(_pd), d_x, n, dim, xtda, d_w, d_y,
                                                    m, ytda, d_s, model_id), self._h)

    def krige_solve(self, kind, eps, nugget, d_x, n, dim, xtda, d_phi, lda, d_w):
        """returns (status, route, mean)"""
        route, mean = C.c_int(0), C.c_double(0)
        st = lib().gsl_sinterp_hip_krige_solve(self._h, kind, eps, nugget, d_x, n, dim, xtda, d_phi, lda, d_w,
                                               C.byref(mean), C.byref(route))
        return st, route.value, mean.value

    def krige_eval(self, kind, eps, mean, d_x, n, dim, xtda, d_w, d_y, m, ytda, d_s, model_id=0):
        check(lib().gsl_sinterp_hip_krige_eval(self._h, kind, eps, mean, d_x, n, dim, xtda, d_w, d_y, m, ytda, d_s,
                                               model_id), self._h)

    def krige_variance_prepare(self, n, d_llt, lda, d_b, d_dinv):
        """b = K^-1 1 -> d_b[n], inverted 32x32 diagonal blocks -> d_dinv[ceil(n/32) * 1024]; returns (status, 1^T b)"""
        denom = C.c_double(0)
        st = lib().gsl_sinterp_hip_krige_variance_prepare(self._h, n, d_llt, lda, d_b, d_dinv, C.byref(denom))
        return st, denom.value

    @staticmethod
    def krige_variance_work(n, chunk):
        """doubles of d_work that krige_variance needs for `chunk` targets per pass"""
        return lib().gsl_sinterp_hip_krige_variance_work(n, chunk)

    def krige_variance(self, kind, eps, d_x, n, dim, xtda, d_llt, lda, d_b, d_dinv, denom, d_y, m, ytda, d_var, d_work, chunk):
        return lib().gsl_sinterp_hip_krige_variance(self._h, kind, eps, d_x, n, dim, xtda, d_llt, lda, d_b, d_dinv, denom,
                                                    d_y, m, ytda, d_var, d_work, chunk)

    def knn(self, d_x, n, dim, xtda, d_y, m, ytda, k, d_idx, d_r2=None, model_id=0):
        """d_idx[m x k] = rows of the k nearest centres of every target, ascending (r2, row); d_r2 optional; returns the status"""
        return lib().gsl_sinterp_hip_knn(self._h, d_x, n, dim, xtda, d_y, m, ytda, k, d_idx, d_r2, model_id)

    def local_krige(self, kind, eps, nugget, d_x, n, dim, xtda, d_f, d_y, m, ytda, k, d_s=None, d_var=None, d_idx=None, model_id=0):
        """ordinary kriging on the k nearest centres of every target; each output optional; synchronises;
        returns (status, failed): GSL_EDOM with `failed` targets NaN where a neighbourhood's matrix has a failed pivot"""
        failed = C.c_size_t(0)
        st = lib().gsl_sinterp_hip_local_krige(self._h, kind, eps, nugget, d_x, n, dim, xtda, d_f, d_y, m, ytda, k, d_s, d_var, d_idx,
                                               C.byref(failed), model_id)
        return st, failed.value

    def local_ukrige(self, kind, eps, nugget, d_x, n, dim, xtda, d_f, d_y, m, ytda, k, d_s=None, d_var=None, d_idx=None, model_id=0):
        """local_krige with a linear drift (k >= dim + 2); returns (status, failed)"""
        failed = C.c_size_t(0)
        st = lib().gsl_sinterp_hip_local_ukrige(self._h, kind, eps, nugget, d_x, n, dim, xtda, d_f, d_y, m, ytda, k, d_s, d_var, d_idx,
                                                C.byref(failed), model_id)
        return st, failed.value

    def local_pack(self, d_x, n, dim, xtda, d_f=None, model_id=0):
        return lib().gsl_sinterp_hip_local_pack(self._h, d_x, n, dim, xtda, d_f, model_id)

    def variogram(self, d_x, n, dim, xtda, d_f, h_max, n_bins):
        """(status, acc [n_bins x 7] uint64, shift [3]): the binned pair sums as exact integers"""
        acc = np.full((max(n_bins, 0), 7), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        shift = (C.c_int * 3)(-1, -1, -1)
        st = lib().gsl_sinterp_hip_variogram(self._h, d_x, n, dim, xtda, d_f, h_max, n_bins,
                                             acc.ctypes.data_as(C.POINTER(C.c_uint64)), shift)
        return st, acc, [int(s) for s in shift]

    def variogram_pairs_tested(self):
        """unordered pairs whose r2 the last variogram call on this context computed"""
        return int(lib().gsl_sinterp_hip_variogram_pairs_tested(self._h))

    def bbox(self, d_x, n, dim, xtda):
        """(status, box [dim x 2]): min and max of every coordinate"""
        box = np.full((dim, 2), np.nan)
        st = lib().gsl_sinterp_hip_bbox(self._h, d_x, n, dim, xtda, box.ctypes.data_as(_pd))
        return st, box

    def local_pack_count(self):
        """how often this context has binned a set of centres for knn / local_krige"""
        return lib().gsl_sinterp_hip_local_pack_count(self._h)

    def shepard_fit(self, d_x, n, dim, xtda, d_f, nq, nw, d_rq, d_rw, d_coef):
        """modified Shepard: radii and the n x nc nodal coefficients; synchronises; returns (status, (linear fallbacks,
        constant fallbacks, coincident nodes)): GSL_EDOM when a node has a coincident site"""
        counts = (C.c_size_t * 3)(0, 0, 0)
        st = lib().gsl_sinterp_hip_shepard_fit(self._h, d_x, n, dim, xtda, d_f, nq, nw, d_rq, d_rw, d_coef, counts)
        return st, tuple(int(v) for v in counts)

    def shepard_eval(self, d_x, n, dim, xtda, d_f, d_rq, d_rw, d_coef, d_y, m, ytda, d_s=None, d_g=None, gtda=0, d_leaf=None, model_id=0):
        """modified Shepard sweep; each output optional; synchronises; returns (status, outside): GSL_EDOM with `outside`
        targets NaN / -1 where no node's radius covers the target"""
        outside = C.c_size_t(0)
        st = lib().gsl_sinterp_hip_shepard_eval(self._h, d_x, n, dim, xtda, d_f, d_rq, d_rw, d_coef, d_y, m, ytda, d_s, d_g, gtda, d_leaf,
                                                C.byref(outside), model_id)
        return st, outside.value

    def shepard_pack_count(self):
        """how often this context has packed a modified Shepard model for evaluation"""
        return lib().gsl_sinterp_hip_shepard_pack_count(self._h)

    def shepard_fit_count(self):
        return lib().gsl_sinterp_hip_shepard_fit_count(self._h)

    @staticmethod
    def chol_inv_diag_work(n, chunk):
        """doubles of d_work that chol_inv_diag needs for `chunk` rows per pass"""
        return lib().gsl_sinterp_hip_chol_inv_diag_work(n, chunk)

    def chol_inv_diag(self, n, d_llt, lda, d_g, d_work, chunk):
        """d_g[i] = ((L L^T)^-1)_ii from the lower triangle of d_llt; returns the status"""
        return lib().gsl_sinterp_hip_chol_inv_diag(self._h, n, d_llt, lda, d_g, d_work, chunk)

    def loo_combine(self, n, nf, d_g, d_b, denom, d_w, ldw, d_e, lde, d_v):
        """leave-one-out residuals d_e (nf columns) and variances d_v from g; d_b = None: the plain rule; returns the status"""
        return lib().gsl_sinterp_hip_loo_combine(self._h, n, nf, d_g, d_b, denom, d_w, ldw, d_e, lde, d_v)

    def score_reduce(self, n, d_llt, lda, d_f, d_w, d_g, d_b, denom, d_out):
        """d_out[0..3] = log|K|, f.w, sum of squared leave-one-out residuals (0 without d_g), count of bad sites, from a
        factor; d_g / d_b may be None; one launch, asynchronous; returns the status"""
        return lib().gsl_sinterp_hip_score_reduce(self._h, n, d_llt, lda, d_f, d_w, d_g, d_b, denom, d_out)

    def gemm_minus(self, m, n, k, d_a, lda, d_b, ldb, b_is_kn, d_c, ldc, lower_only=0):
        check(lib().gsl_sinterp_hip_gemm_minus(self._h, m, n, k, d_a, lda, d_b, ldb, b_is_kn, d_c, ldc, lower_only),
              self._h)

    def synth_unit(self, seed, first, offset, span, d_out, count):
        check(lib().gsl_sinterp_hip_synth_unit(self._h, seed, first, offset, span, d_out, count), self._h)

    def timer_start(self):
        check(lib().gsl_sinterp_hip_timer_start(self._h), self._h)

    def timer_stop(self):
        ms = C.c_float(0)
        check(lib().gsl_sinterp_hip_timer_stop(self._h, C.byref(ms)), self._h)
        return ms.value


# ------------------------------------------------------------------ host tree
class Rng:
    """gsl_rng (mt19937) from the library's compat slice."""

    def __init__(self, seed=0):
        self._h = lib().gsl_rng_alloc(_ptr("gsl_rng_mt19937"))
        lib().gsl_rng_set(self._h, seed)

    def close(self):
        if self._h:
            lib().gsl_rng_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SimplexTree:
    """The reference's simplex_tree_* API (host, 2-D) over numpy arrays."""

    def __init__(self, dim, n_points):
        self._t = lib().simplex_tree_alloc(dim, n_points)
        if not self._t:
            raise GslError(GSL_EUNIMPL, "simplex_tree_alloc")
        self.data = None
        self._mat = None

    def init(self, data=None, vmin=None, vmax=None, flags=0, rng=None):
        self.data = data
        self._mat = as_matrix(data) if data is not None else None
        mn = as_vector(np.ascontiguousarray(vmin, dtype=np.float64)) if vmin is not None else None
        mx = as_vector(np.ascontiguousarray(vmax, dtype=np.float64)) if vmax is not None else None
        return lib().simplex_tree_init(self._t, C.byref(self._mat) if self._mat is not None else None,
                                       C.byref(mn) if mn is not None else None,
                                       C.byref(mx) if mx is not None else None, flags,
                                       rng._h if rng is not None else None)

    def set_data(self, data):
        self.data = data
        self._mat = as_matrix(data)

    @property
    def c(self):
        return self._t.contents

    def _m(self):
        return C.byref(self._mat) if self._mat is not None else None

    def find_leaf(self, point):
        p = np.ascontiguousarray(point, dtype=np.float64)
        return lib().find_leaf(self._t, self._m(), C.byref(as_vector(p)), None)

    def insert_point(self, leaf):
        return lib().insert_point(self._t, leaf, self._m(), None, None)

    def in_hypersphere(self, node, idx):
        return lib().in_hypersphere(self._t, node, self._m(), idx, None)

    def contains_point(self, node, point):
        p = np.ascontiguousarray(point, dtype=np.float64)
        return lib().contains_point(self._t, node, self._m(), C.byref(as_vector(p)), None)

    def interp_point(self, leaf, response, point):
        p = np.ascontiguousarray(point, dtype=np.float64)
        r = as_vector(response) if response is not None else None
        return lib().interp_point(self._t, leaf, self._m(), C.byref(r) if r is not None else None,
                                  C.byref(as_vector(p)), None)

    # flat copies of the DAG arrays
    @property
    def n_nodes(self):
        return self.c.n_simplexes

    def arrays(self):
        t = self.c
        n = t.n_simplexes
        nodes = np.ctypeslib.as_array(C.cast(t.simplexes, C.POINTER(C.c_int)), (n, 3)).copy()
        types = (nodes[:, 2] & 3).astype(np.int32)
        pidx = np.ctypeslib.as_array(t.pidx, (3 * n,)).copy().astype(np.int32)
        links = np.ctypeslib.as_array(t.links, (3 * n,)).copy().astype(np.int32)
        assert (nodes[:, 0] == 3 * np.arange(n)).all() and (nodes[:, 1] == 3 * np.arange(n)).all()
        return types, pidx, links

    def shuffle(self):
        t = self.c
        return np.ctypeslib.as_array(t.shuffle.contents.data, (max(t.max_points, 1),)).copy()[: t.n_points]

    def geom(self):
        t = self.c
        sp = t.seed_points.contents
        seed = np.ctypeslib.as_array(sp.data, (3, sp.tda))[:, :2].copy().reshape(-1)
        sh = np.array([t.shift.contents.data[0], t.shift.contents.data[1]])
        sc = np.array([t.scale.contents.data[0], t.scale.contents.data[1]])
        return np.concatenate([seed, sh, sc])

    def device_alloc(self, device=0):
        h = lib().simplex_tree_device_alloc(self._t, self._m(), device)
        if not h:
            raise GslError(GSL_EFAILED, "simplex_tree_device_alloc")
        return DeviceTree(h)

    def fwrite(self, path):
        with CFile(path, "wb") as fp:
            return lib().simplex_tree_fwrite(fp, self._t)

    @classmethod
    def fread(cls, path, data=None):
        with CFile(path, "rb") as fp:
            t = lib().simplex_tree_fread(fp)
        if not t:
            return None
        self = cls.__new__(cls)
        self._t, self.data, self._mat = t, None, None
        if data is not None:
            self.set_data(data)
        return self

    def output_triangulation(self, response, standardize, lines=None, points=None, circles=None):
        enc = lambda p: str(p).encode() if p is not None else None
        r = as_vector(response) if response is not None else None
        lib().output_triangulation(self._t, self._m(), C.byref(r) if r is not None else None, int(standardize),
                                   enc(lines), enc(points), enc(circles))

    def leaf_walk_order(self):
        """node ids in the order check_leaf_nodes visits them"""
        order = []
        CB = C.CFUNCTYPE(None, _pt, C.c_int)
        cb = CB(lambda tree, node: order.append(node))
        lib().check_leaf_nodes(self._t, C.cast(cb, C.c_void_p))
        return order

    def check_device(self, device=0):
        """(verdict, leaf_violations, delaunay_violations): check_leaf_nodes + check_delaunay on the GPU."""
        lv, dv = C.c_longlong(0), C.c_longlong(0)
        ok = lib().simplex_tree_check_device(self._t, self._m(), device, C.byref(lv), C.byref(dv))
        return ok, lv.value, dv.value

    def device_alloc_multi(self, devices):
        arr = (C.c_int * len(devices))(*devices)
        h = lib().simplex_tree_device_alloc_multi(self._t, self._m(), arr, len(devices))
        if not h:
            raise GslError(GSL_EFAILED, "simplex_tree_device_alloc_multi")
        return DeviceTree(h)

    def close(self):
        if self._t:
            lib().simplex_tree_free(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceTree:
    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    def set_response(self, response):
        return lib().simplex_tree_device_set_response(self._h, C.byref(as_vector(response)))

    def eval_many(self, targets, want_leaf=True, out=None):
        """out = (values, leaf) preallocated arrays (timing loops: fresh arrays pay first-touch page faults in the copy)"""
        m = targets.shape[0]
        vals = np.empty(m, dtype=np.float64) if out is None else out[0]
        leaf = (np.empty(m, dtype=np.int32) if out is None else out[1]) if want_leaf else None
        st = lib().simplex_tree_device_eval_many(self._h, C.byref(as_matrix(targets)), C.byref(as_vector(vals)),
                                                 leaf.ctypes.data_as(_pi) if want_leaf else None)
        return st, vals, leaf

    def eval_resident(self, d_targets, m, ttda, d_values, d_leaf):
        return lib().simplex_tree_device_eval_resident(self._h, d_targets, m, ttda, d_values, d_leaf)

    def set_responses(self, F):
        """F: n_points x K responses (row stride honoured), independent of set_response"""
        return lib().simplex_tree_device_set_responses(self._h, C.byref(as_matrix(F)))

    def n_responses(self):
        return int(lib().simplex_tree_device_n_responses(self._h))

    def eval_fields_many(self, targets, want_grad=False, want_leaf=True, out=None):
        """(status, S [m x K], G [m x K dim] or None, leaf or None) from one locate; out = (S, G or None) preallocated"""
        m, dim, k = targets.shape[0], targets.shape[1], max(self.n_responses(), 1)
        S = np.empty((m, k), dtype=np.float64) if out is None else out[0]
        G = (np.empty((m, k * dim), dtype=np.float64) if out is None else out[1]) if want_grad else None
        leaf = np.empty(m, dtype=np.int32) if want_leaf else None
        st = lib().simplex_tree_device_eval_fields_many(self._h, C.byref(as_matrix(targets)), C.byref(as_matrix(S)),
                                            C.byref(as_matrix(G)) if want_grad else None, leaf.ctypes.data_as(_pi) if want_leaf else None)
        return st, S, G, leaf

    def eval_fields_resident(self, d_targets, m, ttda, d_S, stda, d_G=None, gtda=0, d_leaf=None):
        return lib().simplex_tree_device_eval_fields_resident(self._h, d_targets, m, ttda, d_S, stda, d_G, gtda, d_leaf)

    def n_devices(self):
        return lib().simplex_tree_device_n_devices(self._h)

    def transport(self):
        return lib().simplex_tree_device_transport(self._h).decode()

    def close(self):
        if self._h:
            lib().simplex_tree_device_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SimplexMesh:
    """An imported triangulation (QHull / CGAL style arrays, triangles in 2-D or tetrahedra in 3-D) or the final
    triangulation of a SimplexTree."""

    def __init__(self, handle, keep=None):
        if not handle:
            raise GslError(GSL_EINVAL, "simplex_mesh")
        self._h = C.c_void_p(handle)
        self._keep = keep

    @classmethod
    def from_arrays(cls, points, triangles, neighbours=None):
        """dim = points.shape[1]: 2 -> simplex_mesh_import, anything else -> simplex_mesh_import_nd (3: tetrahedra)"""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        dim = pts.shape[1]
        tri = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, dim + 1)
        nbr = None if neighbours is None else np.ascontiguousarray(neighbours, dtype=np.int32).reshape(-1, dim + 1)
        pn = nbr.ctypes.data_as(_pi) if nbr is not None else None
        if dim == 2:
            h = lib().simplex_mesh_import(C.byref(as_matrix(pts)), tri.ctypes.data_as(_pi), pn, len(tri))
        else:
            h = lib().simplex_mesh_import_nd(C.byref(as_matrix(pts)), dim, tri.ctypes.data_as(_pi), pn, len(tri))
        return cls(h)

    @classmethod
    def from_tree(cls, tree):
        return cls(lib().simplex_mesh_from_tree(tree._t, tree._m()), keep=tree)

    @property
    def n_triangles(self):
        return int(lib().simplex_mesh_n_triangles(self._h))

    def dim(self):
        return int(lib().simplex_mesh_dim(self._h))

    def _ints(self, fn, width):
        p = fn(self._h)
        if not p:
            return None
        n = self.n_triangles
        return np.ctypeslib.as_array(p, shape=(n * width,)).reshape(n, width).copy() if width > 1 else \
            np.ctypeslib.as_array(p, shape=(n,)).copy()

    def triangles(self):
        return self._ints(lib().simplex_mesh_triangles, self.dim() + 1)

    def neighbours(self):
        return self._ints(lib().simplex_mesh_neighbours, self.dim() + 1)

    def tree_nodes(self):
        return self._ints(lib().simplex_mesh_tree_nodes, 1)

    def geometry(self):
        d = self.dim()
        sh, sc = (C.c_double * d)(), (C.c_double * d)()
        lib().simplex_mesh_geometry(self._h, sh, sc)
        return np.array(sh[:]), np.array(sc[:])

    def points(self):
        n, d = int(lib().simplex_mesh_n_points(self._h)), self.dim()
        return np.ctypeslib.as_array(lib().simplex_mesh_points(self._h), shape=(n * d,)).reshape(n, d).copy()

    def bbox(self):
        d = self.dim()
        lo, hi = (C.c_double * d)(), (C.c_double * d)()
        lib().simplex_mesh_bbox(self._h, lo, hi)
        return np.array(lo[:]), np.array(hi[:])

    def set_convex(self, convex):
        lib().simplex_mesh_set_convex(self._h, int(convex))

    def convex(self):
        return bool(lib().simplex_mesh_convex(self._h))

    def delaunay_metric(self):
        """1: Delaunay in the coordinates as given, 2: in the standardised ones, 0: in neither (or a 3-D mesh)"""
        return int(lib().simplex_mesh_delaunay_metric(self._h))

    def vertex_adjacency(self):
        """(offsets [n_points + 1], neighbours): every undirected edge once per endpoint, the neighbours of a vertex ascending"""
        n_points = len(self.points())
        off = np.empty(n_points + 1, dtype=np.int32)
        adj = np.empty(6 * self.n_triangles + 1, dtype=np.int32)
        cnt = C.c_size_t(0)
        st = lib().simplex_mesh_vertex_adjacency(self._h, off.ctypes.data_as(_pi), adj.ctypes.data_as(_pi), len(adj), C.byref(cnt))
        if st != 0:
            raise GslError(st, "simplex_mesh_vertex_adjacency")
        return off, adj[:cnt.value].copy()

    def device_alloc(self, device=0):
        h = lib().simplex_mesh_device_alloc(self._h, device)
        if not h:
            raise GslError(GSL_EFAILED, "simplex_mesh_device_alloc")
        return DeviceMesh(h, self)

    def device_alloc_multi(self, devices):
        arr = (C.c_int * len(devices))(*devices)
        h = lib().simplex_mesh_device_alloc_multi(self._h, arr, len(devices))
        if not h:
            raise GslError(GSL_EFAILED, "simplex_mesh_device_alloc_multi")
        return DeviceMesh(h, self)

    def fwrite(self, path):
        with CFile(path, "wb") as fp:
            return lib().simplex_mesh_fwrite(fp, self._h)

    @classmethod
    def fread(cls, path):
        with CFile(path, "rb") as fp:
            h = lib().simplex_mesh_fread(fp)
        return cls(h) if h else None

    def close(self):
        if self._h:
            lib().simplex_mesh_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceMesh:
    def __init__(self, handle, mesh):
        self._h = C.c_void_p(handle)
        self._mesh = mesh

    def set_response(self, response):
        return lib().simplex_mesh_device_set_response(self._h, C.byref(as_vector(response)))

    def eval_many(self, targets, out=None):
        m = targets.shape[0]
        vals = np.empty(m, dtype=np.float64) if out is None else out[0]
        tri = np.empty(m, dtype=np.int32) if out is None else out[1]
        st = lib().simplex_mesh_device_eval_many(self._h, C.byref(as_matrix(targets)), C.byref(as_vector(vals)), tri.ctypes.data_as(_pi))
        return st, vals, tri

    def eval_natural_many(self, targets, out=None):
        """natural-neighbour (Sibson) values on a 2-D Delaunay mesh; same shapes as eval_many"""
        m = targets.shape[0]
        vals = np.empty(m, dtype=np.float64) if out is None else out[0]
        tri = np.empty(m, dtype=np.int32) if out is None else out[1]
        st = lib().simplex_mesh_device_eval_natural_many(self._h, C.byref(as_matrix(targets)), C.byref(as_vector(vals)),
                                                         tri.ctypes.data_as(_pi))
        return st, vals, tri

    def bind_gradients(self, gradients=None):
        """Clough-Tocher: the n_points x 2 gradients to interpolate; None = estimate them at the first cubic call"""
        return lib().simplex_mesh_device_bind_gradients(self._h, C.byref(as_matrix(gradients)) if gradients is not None else None)

    def set_gradient_options(self, rtol, maxiter):
        return lib().simplex_mesh_device_set_gradient_options(self._h, rtol, maxiter)

    def gradients(self):
        """(status, g [n_points x 2], iterations, residual) of the gradients in use (estimates them now if still to do)"""
        g = np.empty((self._mesh.points().shape[0], 2), dtype=np.float64)
        it, res = C.c_size_t(0), C.c_double(0.0)
        st = lib().simplex_mesh_device_gradients(self._h, C.byref(as_matrix(g)), C.byref(it), C.byref(res))
        return st, g, it.value, res.value

    def eval_cubic_many(self, targets, want_grad=False):
        """(status, values, gradient or None, triangle): Clough-Tocher values (and grad s) on a 2-D mesh"""
        m = targets.shape[0]
        vals = np.empty(m, dtype=np.float64)
        grad = np.empty((m, 2), dtype=np.float64) if want_grad else None
        tri = np.empty(m, dtype=np.int32)
        st = lib().simplex_mesh_device_eval_cubic_many(self._h, C.byref(as_matrix(targets)), C.byref(as_vector(vals)),
                                                       C.byref(as_matrix(grad)) if want_grad else None, tri.ctypes.data_as(_pi))
        return st, vals, grad, tri

    def eval_cubic_resident(self, d_targets, m, ttda, d_values, d_grad=None, gtda=2, d_tri=None):
        return lib().simplex_mesh_device_eval_cubic_resident(self._h, d_targets, m, ttda, d_values, d_grad, gtda, d_tri)

    def set_responses(self, F):
        """F: n_points x K responses (row stride honoured), independent of set_response"""
        return lib().simplex_mesh_device_set_responses(self._h, C.byref(as_matrix(F)))

    def n_responses(self):
        return int(lib().simplex_mesh_device_n_responses(self._h))

    def eval_fields_many(self, targets, want_grad=False, want_leaf=True, out=None):
        """(status, S [m x K], G [m x K dim] or None, leaf or None) from one locate; out = (S, G or None) preallocated"""
        m, dim, k = targets.shape[0], targets.shape[1], max(self.n_responses(), 1)
        S = np.empty((m, k), dtype=np.float64) if out is None else out[0]
        G = (np.empty((m, k * dim), dtype=np.float64) if out is None else out[1]) if want_grad else None
        leaf = np.empty(m, dtype=np.int32) if want_leaf else None
        st = lib().simplex_mesh_device_eval_fields_many(self._h, C.byref(as_matrix(targets)), C.byref(as_matrix(S)),
                                            C.byref(as_matrix(G)) if want_grad else None, leaf.ctypes.data_as(_pi) if want_leaf else None)
        return st, S, G, leaf

    def eval_fields_resident(self, d_targets, m, ttda, d_S, stda, d_G=None, gtda=0, d_leaf=None):
        return lib().simplex_mesh_device_eval_fields_resident(self._h, d_targets, m, ttda, d_S, stda, d_G, gtda, d_leaf)

    def n_devices(self):
        return lib().simplex_mesh_device_n_devices(self._h)

    def eval_resident(self, d_targets, m, ttda, d_values, d_tri):
        return lib().simplex_mesh_device_eval_resident(self._h, d_targets, m, ttda, d_values, d_tri)

    def eval_natural_resident(self, d_targets, m, ttda, d_values, d_tri):
        return lib().simplex_mesh_device_eval_natural_resident(self._h, d_targets, m, ttda, d_values, d_tri)

    def ctx_handle(self):
        return lib().simplex_mesh_device_ctx(self._h)

    def close(self):
        if self._h:
            lib().simplex_mesh_device_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ facade
class Sinterp:
    TYPES = {"gaussian": "gsl_sinterp_rbf_gaussian", "tps": "gsl_sinterp_rbf_tps", "tps_affine": "gsl_sinterp_rbf_tps_affine",
             "wendland": "gsl_sinterp_rbf_wendland", "linear_mesh": "gsl_sinterp_linear_mesh",
             "natural_mesh": "gsl_sinterp_natural_mesh", "natural_simplex": "gsl_sinterp_natural_simplex",
             "cubic_mesh": "gsl_sinterp_cubic_mesh", "cubic_simplex": "gsl_sinterp_cubic_simplex",
             "linear_simplex": "gsl_sinterp_linear_simplex", "kriging": "gsl_sinterp_kriging",
             "matern32": "gsl_sinterp_rbf_matern32", "matern52": "gsl_sinterp_rbf_matern52", "imq": "gsl_sinterp_rbf_imq",
             "kriging_matern32": "gsl_sinterp_kriging_matern32", "kriging_matern52": "gsl_sinterp_kriging_matern52"}

    MORE_TYPES = {"shepard": "gsl_sinterp_shepard"}    # consulted after TYPES

    def __init__(self, kind, dim, size, device=0):
        self._p = lib().gsl_sinterp_alloc(_ptr(self.TYPES[kind] if kind in self.TYPES else self.MORE_TYPES[kind]), dim, size)
        if not self._p:
            raise GslError(GSL_EINVAL, "gsl_sinterp_alloc")
        lib().gsl_sinterp_set_device(self._p, device)
        self._rng = None

    def set_shape(self, eps):
        return lib().gsl_sinterp_set_shape(self._p, eps)

    def set_nugget(self, nugget):
        return lib().gsl_sinterp_set_nugget(self._p, nugget)

    def mean(self):
        v = C.c_double(0)
        st = lib().gsl_sinterp_mean(self._p, C.byref(v))
        return st, v.value

    def set_drift(self, order):
        """kriging, before init: 0 = ordinary kriging, 1 / 2 = universal kriging with a linear / quadratic drift"""
        return lib().gsl_sinterp_set_drift(self._p, int(order))

    def drift(self):
        return lib().gsl_sinterp_drift(self._p)

    @staticmethod
    def drift_terms(dim, order):
        return lib().gsl_sinterp_drift_terms(dim, order)

    def drift_coefficients(self, field=0):
        """(status, c[q], shift[dim], scale[dim]) of an interpolant initialised with a drift"""
        dim = self._p.contents.dim
        q = max(int(self.drift_terms(dim, self.drift())), 1)
        c, shift, scale = np.full(q, np.nan), np.full(dim, np.nan), np.full(dim, np.nan)
        st = lib().gsl_sinterp_drift_coefficients(self._p, field, C.byref(as_vector(c)), C.byref(as_vector(shift)), C.byref(as_vector(scale)))
        return st, c, shift, scale

    def set_variance(self, want=True):
        """kriging: the next init keeps the Cholesky factor (N^2 doubles on the device) for eval_variance_*"""
        return lib().gsl_sinterp_set_variance(self._p, int(want))

    def eval_variance_e(self, y):
        out = C.c_double(0)
        st = lib().gsl_sinterp_eval_variance_e(self._p, C.byref(as_vector(np.ascontiguousarray(y, dtype=np.float64))),
                                               C.byref(out))
        return st, out.value

    def eval_variance_many(self, y, out=None):
        """kriging variance sigma^2 at the rows of y (clamped at 0); returns (status, values)"""
        v = np.empty(y.shape[0], dtype=np.float64) if out is None else out
        st = lib().gsl_sinterp_eval_variance_many(self._p, C.byref(as_matrix(y)), C.byref(as_vector(v)))
        return st, v

    def eval_variance_resident(self, d_y, m, ytda, d_var):
        return lib().gsl_sinterp_eval_variance_resident(self._p, d_y, m, ytda, d_var)

    def eval_covariance_many(self, ya, yb=None, out=None):
        """joint posterior covariance of the rows of ya with the rows of yb (None: ya, symmetric to the bit), not clamped;
        returns (status, Cov ma x mb)"""
        mb = ya.shape[0] if yb is None else yb.shape[0]
        cov = np.full((ya.shape[0], mb), np.nan) if out is None else out
        st = lib().gsl_sinterp_eval_covariance_many(self._p, C.byref(as_matrix(ya)), None if yb is None else C.byref(as_matrix(yb)),
                                                    C.byref(as_matrix(cov)))
        return st, cov

    def eval_covariance_resident(self, d_ya, ma, yatda, d_yb, mb, ybtda, d_cov, ctda):
        return lib().gsl_sinterp_eval_covariance_resident(self._p, d_ya, ma, yatda, d_yb, mb, ybtda, d_cov, ctda)

    def simulate_many(self, y, sigma2, jitter, zn, out=None):
        """conditional draws at the rows of y from the caller's standard normals zn (m x S): mean + sqrt(sigma2) chol(Sigma +
        jitter I) zn; returns (status, Out m x S)"""
        o = np.full(zn.shape, np.nan) if out is None else out
        st = lib().gsl_sinterp_simulate_many(self._p, C.byref(as_matrix(y)), sigma2, jitter, C.byref(as_matrix(zn)), C.byref(as_matrix(o)))
        return st, o

    def simulate_resident(self, d_y, m, ytda, sigma2, jitter, d_zn, ztda, n_draws, d_out, otda):
        return lib().gsl_sinterp_simulate_resident(self._p, d_y, m, ytda, sigma2, jitter, d_zn, ztda, n_draws, d_out, otda)

    def set_neighbours(self, k):
        """kriging: k > 0 = the next init takes the local route (kriging on the k nearest centres of every target), 0 = global"""
        return lib().gsl_sinterp_set_neighbours(self._p, int(k))

    def eval_local_many(self, y, want_s=True, want_var=True, want_idx=True):
        """(status, s, var, idx) of the local route from one pass; an output that is not wanted is None"""
        m, k = y.shape[0], int(self._p.contents.neighbours)
        s = np.full(m, np.nan) if want_s else None
        v = np.full(m, np.nan) if want_var else None
        idx = np.full((m, max(k, 1)), -1, dtype=np.int32) if want_idx else None
        st = lib().gsl_sinterp_eval_local_many(self._p, C.byref(as_matrix(y)), C.byref(as_vector(s)) if want_s else None,
                                               C.byref(as_vector(v)) if want_var else None,
                                               idx.ctypes.data_as(_pi) if want_idx else None)
        return st, s, v, idx

    def set_shepard(self, nq=0, nw=0):
        """modified Shepard, before init: neighbours behind the fit radius and the weight radius; 0 = Renka's defaults"""
        return lib().gsl_sinterp_set_shepard(self._p, int(nq), int(nw))

    def shepard_stats(self):
        """(status, linear fallbacks, constant fallbacks, largest radius of influence) after init"""
        nl, ncst, rw = C.c_size_t(0), C.c_size_t(0), C.c_double(float("nan"))
        st = lib().gsl_sinterp_shepard_stats(self._p, C.byref(nl), C.byref(ncst), C.byref(rw))
        return st, nl.value, ncst.value, rw.value

    def shepard_counters(self):
        """(fits, packs) of the interpolant's device context; (0, 0) before the first init"""
        h = lib().gsl_sinterp_shepard_ctx(self._p)
        return int(lib().gsl_sinterp_hip_shepard_fit_count(h)), int(lib().gsl_sinterp_hip_shepard_pack_count(h))

    def set_loo(self, want=True):
        """positive definite RBF types and kriging: the next init computes the leave-one-out residuals and variances"""
        return lib().gsl_sinterp_set_loo(self._p, int(want))

    def loo_residuals(self, out=None):
        """(status, E): the size x K leave-one-out residuals f_i - s^(-i)(x_i); out = preallocated E (row stride honoured)"""
        E = np.full((self._p.contents.size, max(self.n_fields(), 1)), np.nan) if out is None else out
        st = lib().gsl_sinterp_loo_residuals(self._p, C.byref(as_matrix(E)))
        return st, E

    def loo_variance(self, out=None):
        """(status, v): the leave-one-out variances"""
        v = np.full(self._p.contents.size, np.nan) if out is None else out
        st = lib().gsl_sinterp_loo_variance(self._p, C.byref(as_vector(v)))
        return st, v

    def eval_grad_e(self, y):
        """(status, s, g): value and gradient (dim entries) at one target; NaN on failure"""
        out = C.c_double(0)
        g = np.empty(self._p.contents.dim, dtype=np.float64)
        st = lib().gsl_sinterp_eval_grad_e(self._p, C.byref(as_vector(np.ascontiguousarray(y, dtype=np.float64))), C.byref(out),
                                           C.byref(as_vector(g)))
        return st, out.value, g

    def eval_grad_many(self, y, want_value=True, out=None):
        """(status, s or None, g): values and the m x dim gradient at the rows of y; out = (s or None, g) preallocated"""
        m = y.shape[0]
        s = (np.empty(m, dtype=np.float64) if out is None else out[0]) if want_value else None
        g = np.empty((m, self._p.contents.dim), dtype=np.float64) if out is None else out[1]
        st = lib().gsl_sinterp_eval_grad_many(self._p, C.byref(as_matrix(y)), C.byref(as_vector(s)) if want_value else None,
                                              C.byref(as_matrix(g)))
        return st, s, g

    def eval_grad_resident(self, d_y, m, ytda, d_s, d_g, gtda):
        return lib().gsl_sinterp_eval_grad_resident(self._p, d_y, m, ytda, d_s, d_g, gtda)

    def init_fields(self, x, F):
        """F: size x K responses (row stride honoured); one weight vector per column"""
        return lib().gsl_sinterp_init_fields(self._p, C.byref(as_matrix(x)), C.byref(as_matrix(F)))

    def n_fields(self):
        return int(lib().gsl_sinterp_n_fields(self._p))

    def eval_fields_e(self, y):
        """(status, s): the K values at one target; NaN on failure"""
        s = np.full(max(self.n_fields(), 1), np.nan)
        st = lib().gsl_sinterp_eval_fields_e(self._p, C.byref(as_vector(np.ascontiguousarray(y, dtype=np.float64))), C.byref(as_vector(s)))
        return st, s

    def eval_fields_many(self, y, out=None):
        """(status, S): the m x K values at the rows of y; out = preallocated S (row stride honoured)"""
        S = np.empty((y.shape[0], max(self.n_fields(), 1)), dtype=np.float64) if out is None else out
        st = lib().gsl_sinterp_eval_fields_many(self._p, C.byref(as_matrix(y)), C.byref(as_matrix(S)))
        return st, S

    def eval_fields_resident(self, d_y, m, ytda, d_s, stda):
        return lib().gsl_sinterp_eval_fields_resident(self._p, d_y, m, ytda, d_s, stda)

    def linear_init_fields(self, x, F):
        """the linear types: F is size x K (row stride honoured); field 0 is the interpolant of every other entry"""
        return lib().gsl_sinterp_linear_init_fields(self._p, C.byref(as_matrix(x)), C.byref(as_matrix(F)))

    def linear_eval_fields_e(self, y, want_grad=False):
        """(status, s [K], g [K x dim] or None) at one target; NaN on failure"""
        k = max(self.n_fields(), 1)
        s = np.full(k, np.nan)
        g = np.full((k, self._p.contents.dim), np.nan) if want_grad else None
        st = lib().gsl_sinterp_linear_eval_fields_e(self._p, C.byref(as_vector(np.ascontiguousarray(y, dtype=np.float64))), C.byref(as_vector(s)),
                                                    C.byref(as_matrix(g)) if want_grad else None)
        return st, s, g

    def linear_eval_fields_many(self, y, want_grad=False, want_leaf=False, out=None):
        """(status, S [m x K], G [m x K dim] or None, leaf or None) from one locate; out = (S, G or None) preallocated
        (row strides honoured)"""
        m, k = y.shape[0], max(self.n_fields(), 1)
        S = np.empty((m, k), dtype=np.float64) if out is None else out[0]
        G = (np.empty((m, k * self._p.contents.dim), dtype=np.float64) if out is None else out[1]) if want_grad else None
        leaf = np.empty(m, dtype=np.int32) if want_leaf else None
        st = lib().gsl_sinterp_linear_eval_fields_many(self._p, C.byref(as_matrix(y)), C.byref(as_matrix(S)),
                                                       C.byref(as_matrix(G)) if want_grad else None,
                                                       leaf.ctypes.data_as(_pi) if want_leaf else None)
        return st, S, G, leaf

    def linear_eval_fields_resident(self, d_y, m, ytda, d_S, stda, d_G=None, gtda=0, d_leaf=None):
        return lib().gsl_sinterp_linear_eval_fields_resident(self._p, d_y, m, ytda, d_S, stda, d_G, gtda, d_leaf)

    def field_weights(self, q):
        w = np.empty(self._p.contents.size, dtype=np.float64)
        st = lib().gsl_sinterp_get_field_weights(self._p, q, C.byref(as_vector(w)))
        return st, w

    def field_mean(self, q):
        v = C.c_double(0)
        st = lib().gsl_sinterp_field_mean(self._p, q, C.byref(v))
        return st, v.value

    def field_poly(self, q):
        c = np.zeros(self._p.contents.dim + 1, dtype=np.float64)
        st = lib().gsl_sinterp_field_poly(self._p, q, C.byref(as_vector(c)))
        return st, c

    def poly(self):
        c = np.zeros(self._p.contents.dim + 1, dtype=np.float64)
        st = lib().gsl_sinterp_poly(self._p, C.byref(as_vector(c)))
        return st, c

    def set_solver(self, solver):
        return lib().gsl_sinterp_set_solver(self._p, solver)

    def set_rcond(self, want=True):
        return lib().gsl_sinterp_set_rcond(self._p, int(want))

    def rcond(self):
        r = C.c_double(0)
        st = lib().gsl_sinterp_rcond(self._p, C.byref(r))
        return st, r.value

    def route(self):
        return lib().gsl_sinterp_route(self._p)

    def set_devices(self, n):
        return lib().gsl_sinterp_set_devices(self._p, n)

    def set_device_list(self, devices):
        arr = (C.c_int * len(devices))(*devices)
        return lib().gsl_sinterp_set_device_list(self._p, arr, len(devices))

    def n_devices(self):
        return lib().gsl_sinterp_n_devices(self._p)

    def set_triangulation(self, triangles, neighbours=None):
        w = int(self._p.contents.dim) + 1                  # ids per simplex: triangles in 2-D, tetrahedra in 3-D
        tri = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, w)
        nbr = None if neighbours is None else np.ascontiguousarray(neighbours, dtype=np.int32).reshape(-1, w)
        return lib().gsl_sinterp_set_triangulation(self._p, tri.ctypes.data_as(_pi), nbr.ctypes.data_as(_pi) if nbr is not None else None,
                                                   len(tri))

    def set_gradients(self, gradients):
        """Clough-Tocher types, before init: the size x 2 gradients to interpolate (None: back to the estimate)"""
        return lib().gsl_sinterp_set_gradients(self._p, C.byref(as_matrix(gradients)) if gradients is not None else None)

    def set_gradient_options(self, rtol, maxiter):
        return lib().gsl_sinterp_set_gradient_options(self._p, rtol, maxiter)

    def get_gradients(self):
        """(status, g [size x 2], iterations, residual) after init"""
        g = np.empty((self._p.contents.size, self._p.contents.dim if self.name() == "modified-quadratic-shepard" else 2), dtype=np.float64)
        it, res = C.c_size_t(0), C.c_double(0.0)
        st = lib().gsl_sinterp_get_gradients(self._p, C.byref(as_matrix(g)), C.byref(it), C.byref(res))
        return st, g, it.value, res.value

    def set_tree_options(self, flags, rng):
        self._rng = rng
        return lib().gsl_sinterp_set_tree_options(self._p, flags, rng._h if rng is not None else None)

    def init(self, x, f):
        return lib().gsl_sinterp_init(self._p, C.byref(as_matrix(x)), C.byref(as_vector(f)))

    def name(self):
        return lib().gsl_sinterp_name(self._p).decode()

    def eval_e(self, y):
        out = C.c_double(0)
        st = lib().gsl_sinterp_eval_e(self._p, C.byref(as_vector(np.ascontiguousarray(y, dtype=np.float64))),
                                      C.byref(out))
        return st, out.value

    def eval_many(self, y, want_leaf=False, out=None):
        m = y.shape[0]
        s = np.empty(m, dtype=np.float64) if out is None else out
        leaf = np.empty(m, dtype=np.int32) if want_leaf else None
        st = lib().gsl_sinterp_eval_many(self._p, C.byref(as_matrix(y)), C.byref(as_vector(s)),
                                         leaf.ctypes.data_as(_pi) if want_leaf else None)
        return st, s, leaf

    def eval_resident(self, d_y, m, ytda, d_s, d_leaf=None):
        return lib().gsl_sinterp_eval_resident(self._p, d_y, m, ytda, d_s, d_leaf)

    def eval_grid(self, vmin, vmax, n0, n1):
        grid = np.empty((n0, n1), dtype=np.float64)
        st = lib().gsl_sinterp_eval_grid(self._p, C.byref(as_vector(np.ascontiguousarray(vmin, dtype=np.float64))),
                                         C.byref(as_vector(np.ascontiguousarray(vmax, dtype=np.float64))),
                                         C.byref(as_matrix(grid)))
        return st, grid

    def fwrite(self, path):
        with CFile(path, "wb") as fp:
            return lib().gsl_sinterp_fwrite(fp, self._p)

    def fread(self, path):
        with CFile(path, "rb") as fp:
            return lib().gsl_sinterp_fread(fp, self._p)

    def weights(self):
        w = np.empty(self._p.contents.size, dtype=np.float64)
        st = lib().gsl_sinterp_get_weights(self._p, C.byref(as_vector(w)))
        return st, w

    def fit_workspace(self, x, f):
        """a SinterpFit for this interpolant's type, dim, size and (first) device; the interpolant is not changed"""
        return SinterpFit(self, x, f)

    def close(self):
        if self._p:
            lib().gsl_sinterp_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ model selection
class SinterpFit:
    """gsl_sinterp_fit_workspace: likelihood / leave-one-out scores of (eps, nugget) and the 1-D searches over either,
    with the centres, the response and the N x N matrix resident on the device.  Raises GslError with the status of
    gsl_sinterp_fit_alloc when no workspace comes back."""
    LOO, ML = FIT_LOO, FIT_ML

    def __init__(self, interp, x, f):
        self._h = None
        with ErrorCalls() as calls:
            h = lib().gsl_sinterp_fit_alloc(interp._p if interp is not None else None,
                                            C.byref(as_matrix(x)) if x is not None else None,
                                            C.byref(as_vector(f)) if f is not None else None)
        if not h:
            raise GslError(calls[-1][1] if calls else GSL_FAILURE, calls[-1][0] if calls else "gsl_sinterp_fit_alloc")
        self._h = C.c_void_p(h)

    def score(self, criterion, eps, nugget=0.0):
        """(status, score): +inf for a candidate whose matrix does not factor (status 0), NaN on a real failure"""
        v = C.c_double(0)
        st = lib().gsl_sinterp_fit_score(self._h, criterion, eps, nugget, C.byref(v))
        return st, v.value

    def fit_shape(self, criterion, eps_lo, eps_hi, nugget=0.0):
        """(status, eps_best, score_best)"""
        p, v = C.c_double(0), C.c_double(0)
        st = lib().gsl_sinterp_fit_shape(self._h, criterion, nugget, eps_lo, eps_hi, C.byref(p), C.byref(v))
        return st, p.value, v.value

    def fit_nugget(self, criterion, eps, nugget_lo, nugget_hi):
        """(status, nugget_best, score_best)"""
        p, v = C.c_double(0), C.c_double(0)
        st = lib().gsl_sinterp_fit_nugget(self._h, criterion, eps, nugget_lo, nugget_hi, C.byref(p), C.byref(v))
        return st, p.value, v.value

    def set_search(self, n_grid=9, tol=1e-2, max_eval=40):
        return lib().gsl_sinterp_fit_set_search(self._h, n_grid, tol, max_eval)

    def n_eval(self):
        return int(lib().gsl_sinterp_fit_n_eval(self._h))

    def trace(self):
        """(status, params, scores) of the last search, in order of evaluation"""
        k = self.n_eval()
        p, v = np.full(k, np.nan), np.full(k, np.nan)
        st = lib().gsl_sinterp_fit_trace(self._h, C.byref(as_vector(p)), C.byref(as_vector(v)))
        return st, p, v

    def sigma2(self):
        """(status, f.w / N of the last finite score handed back)"""
        v = C.c_double(0)
        st = lib().gsl_sinterp_fit_sigma2(self._h, C.byref(v))
        return st, v.value

    def close(self):
        if self._h:
            lib().gsl_sinterp_fit_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ empirical variogram
def variogram_fit_model(kind, weights, lag, gamma, count, eps_lo, eps_hi, n_grid=0, tol=0.0, max_eval=0):
    """gsl_sinterp_variogram_fit_model on host arrays (no device): (status, eps, c0, c, wss); 0 selects a search default"""
    lag, gamma, count = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (lag, gamma, count))
    out = [C.c_double(0) for _ in range(4)]
    st = lib().gsl_sinterp_variogram_fit_model(kind, weights, *(None if a is None else a.ctypes.data_as(_pd) for a in (lag, gamma, count)),
                                               0 if lag is None else lag.shape[0], eps_lo, eps_hi, n_grid, tol, max_eval,
                                               *(C.byref(o) for o in out))
    return (st, *(o.value for o in out))


def variogram_fit_model_trace():
    """(status, eps, wss): the evaluations of the last variogram_fit_model call, in order"""
    k = int(lib().gsl_sinterp_variogram_fit_model_n_eval())
    p, v = np.full(k, np.nan), np.full(k, np.nan)
    st = lib().gsl_sinterp_variogram_fit_model_trace(C.byref(as_vector(p)), C.byref(as_vector(v)))
    return st, p, v


class Variogram:
    """gsl_sinterp_variogram: the empirical semivariogram of (x, f) as exact binned pair sums from the device, the
    covariance model fitted to it on the host, and its transfer to a kriging interpolant.  Raises GslError with the status
    of gsl_sinterp_variogram_alloc when no workspace comes back."""
    MATHERON, CRESSIE = VARIOGRAM_MATHERON, VARIOGRAM_CRESSIE
    W_COUNT, W_COUNT_H2, W_NONE = VARIOGRAM_W_COUNT, VARIOGRAM_W_COUNT_H2, VARIOGRAM_W_NONE

    def __init__(self, dim, n_bins, device=None):
        self._h = None
        with ErrorCalls() as calls:
            h = lib().gsl_sinterp_variogram_alloc(dim, n_bins)
        if not h:
            raise GslError(calls[-1][1] if calls else GSL_FAILURE, calls[-1][0] if calls else "gsl_sinterp_variogram_alloc")
        self._h = C.c_void_p(h)
        self.n_bins = n_bins
        if device is not None:
            lib().gsl_sinterp_variogram_set_device(self._h, device)

    def set_device(self, device):
        return lib().gsl_sinterp_variogram_set_device(self._h, device)

    def compute(self, x, f, h_max=0.0):
        return lib().gsl_sinterp_variogram_compute(self._h, C.byref(as_matrix(x)) if x is not None else None,
                                                   C.byref(as_vector(f)) if f is not None else None, h_max)

    def compute_resident(self, d_x, n, xtda, d_f, h_max=0.0):
        return lib().gsl_sinterp_variogram_compute_resident(self._h, d_x, n, xtda, d_f, h_max)

    def h_max(self):
        return lib().gsl_sinterp_variogram_h_max(self._h)

    def get(self, estimator=VARIOGRAM_MATHERON):
        """(status, lag, gamma, count); an empty bin has NaN, NaN, 0"""
        lag, gamma, count = (np.full(self.n_bins, np.nan) for _ in range(3))
        st = lib().gsl_sinterp_variogram_get(self._h, estimator, C.byref(as_vector(lag)), C.byref(as_vector(gamma)), C.byref(as_vector(count)))
        return st, lag, gamma, count

    def fit(self, kind, estimator=VARIOGRAM_MATHERON, weights=VARIOGRAM_W_COUNT_H2, eps_lo=0.0, eps_hi=0.0):
        """(status, eps, nugget = c0 / c, sigma2 = c, wss) for the kriging type named `kind` as in Sinterp.TYPES"""
        T = _ptr(Sinterp.TYPES[kind] if kind in Sinterp.TYPES else Sinterp.MORE_TYPES[kind]) if kind is not None else None
        out = [C.c_double(0) for _ in range(4)]
        st = lib().gsl_sinterp_variogram_fit(self._h, T, estimator, weights, eps_lo, eps_hi, *(C.byref(o) for o in out))
        return (st, *(o.value for o in out))

    def apply(self, interp):
        """set_shape + set_nugget of the last fit on a Sinterp"""
        return lib().gsl_sinterp_variogram_apply(self._h, interp._p if interp is not None else None)

    def close(self):
        if self._h:
            lib().gsl_sinterp_variogram_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
