"""ctypes binding of liborbgpu.so (include/orbgpu.h).

The library is the product: there is no Python or CPU fallback.  If the shared object is missing,
or no HIP device is visible, calls fail loudly (OrbGpuError / OSError).
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liborbgpu.so")

OK, EINVAL, ENOMEM, EHIP, ECAPACITY, ELEVEL = 0, -1, -2, -3, -4, -5
MAX_LEVELS = 16
GRID_COLS, GRID_ROWS = 64, 48
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
     ("octave", "<i4"), ("class_id", "<i4")])
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])

DBG_PYRAMID_PADDED, DBG_BLURRED_PADDED, DBG_CANDIDATES, DBG_SELECTED, DBG_GRAPH_COUNTS = 0, 1, 2, 3, 4


class OrbGpuError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("orbgpu status %d: %s" % (status, msg))
        self.status = status


class ExtractorParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("device_id", C.c_int32),
                ("max_batch", C.c_int32)]


class FrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("kp_x", C.c_void_p), ("kp_y", C.c_void_p), ("kp_octave", C.c_void_p),
                ("kp_angle", C.c_void_p), ("u_right", C.c_void_p), ("desc", C.c_void_p),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("grid_inv_w", C.c_float), ("grid_inv_h", C.c_float), ("scale_factors", C.c_void_p),
                ("nlevels", C.c_int32), ("cell_start", C.c_void_p), ("cell_items", C.c_void_p)]


class MapPointView(C.Structure):
    _fields_ = [("m", C.c_int32), ("in_view", C.c_void_p), ("bad", C.c_void_p), ("obs_pos", C.c_void_p),
                ("level", C.c_void_p), ("view_cos", C.c_void_p), ("proj_x", C.c_void_p),
                ("proj_y", C.c_void_p), ("proj_xr", C.c_void_p), ("desc", C.c_void_p)]


class KeyFrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("has_mp", C.c_void_p), ("bad", C.c_void_p), ("already_found", C.c_void_p),
                ("world_pos", C.c_void_p), ("min_dist_inv", C.c_void_p), ("max_dist_inv", C.c_void_p),
                ("max_dist", C.c_void_p), ("desc", C.c_void_p), ("kp_angle", C.c_void_p)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("dist", C.c_float * 5),
                ("mbf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float)]


class DeviceFrameView(C.Structure):
    _fields_ = [("cap", C.c_int32), ("n", C.c_void_p), ("kps", C.c_void_p), ("desc", C.c_void_p),
                ("u_right", C.c_void_p), ("cell_start", C.c_void_p), ("cell_items", C.c_void_p),
                ("nlevels", C.c_int32), ("scale_factors", C.c_void_p), ("min_x", C.c_float), ("max_x", C.c_float),
                ("min_y", C.c_float), ("max_y", C.c_float)]


class DeviceMapPointTable(C.Structure):
    _fields_ = [("m", C.c_int32), ("world_pos", C.c_void_p), ("normal", C.c_void_p), ("min_dist", C.c_void_p),
                ("max_dist", C.c_void_p), ("desc", C.c_void_p), ("skip", C.c_void_p), ("obs_pos", C.c_void_p)]


class LocalPointsProblem(C.Structure):
    _fields_ = [("frame", C.c_void_p), ("table", C.c_void_p), ("Tcw", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float), ("log_scale_factor", C.c_float),
                ("d_kp_to_mp", C.c_void_p), ("d_counts", C.c_void_p), ("d_track", C.c_void_p)]


class DeviceLastFrameView(C.Structure):
    _fields_ = [("cap", C.c_int32), ("n", C.c_void_p), ("kps", C.c_void_p), ("has_mp", C.c_void_p),
                ("outlier", C.c_void_p), ("obs_pos", C.c_void_p), ("world_pos", C.c_void_p), ("desc", C.c_void_p)]


class TrackScratch(C.Structure):
    _fields_ = [("in_view", C.c_void_p), ("proj_x", C.c_void_p), ("proj_y", C.c_void_p), ("proj_xr", C.c_void_p),
                ("view_cos", C.c_void_p), ("level", C.c_void_p)]


class PointsView(C.Structure):
    _fields_ = [("m", C.c_int32), ("bad", C.c_void_p), ("world_pos", C.c_void_p), ("normal", C.c_void_p),
                ("min_dist", C.c_void_p), ("max_dist", C.c_void_p), ("desc", C.c_void_p)]


class LastFrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("has_mp", C.c_void_p), ("outlier", C.c_void_p), ("obs_pos", C.c_void_p),
                ("world_pos", C.c_void_p), ("desc", C.c_void_p), ("kp_octave", C.c_void_p),
                ("kp_angle", C.c_void_p), ("Tcw", C.c_void_p)]


class PoseResult(C.Structure):
    _fields_ = [("Tcw_d", C.c_double * 16), ("Tcw", C.c_float * 16), ("n_initial", C.c_int32), ("n_inliers", C.c_int32),
                ("rounds", C.c_int32), ("iterations", C.c_int32), ("trials", C.c_int32), ("n_bad_index", C.c_int32)]

    def as_dict(self):
        return {"Tcw_d": np.array(self.Tcw_d, np.float64).reshape(4, 4), "Tcw": np.array(self.Tcw, np.float32).reshape(4, 4),
                "n_initial": self.n_initial, "n_inliers": self.n_inliers, "rounds": self.rounds,
                "iterations": self.iterations, "trials": self.trials, "n_bad_index": self.n_bad_index}


class PoseProblem(C.Structure):
    _fields_ = [("frame", C.c_void_p), ("d_kp_to_mp", C.c_void_p), ("d_world_pos", C.c_void_p), ("rows", C.c_int32),
                ("Tcw", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float), ("d_outlier", C.c_void_p),
                ("d_result", C.c_void_p)]


class LocalBAResult(C.Structure):
    _fields_ = [("chi2_start", C.c_double * 2), ("chi2_end", C.c_double * 2), ("n_edges", C.c_int32), ("n_erased", C.c_int32),
                ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("rounds", C.c_int32), ("stopped", C.c_int32),
                ("n_bad_index", C.c_int32), ("reduced_in_lds", C.c_int32)]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("n_edges", "n_erased", "rounds", "stopped", "n_bad_index", "reduced_in_lds")}
        d.update(chi2_start=list(self.chi2_start), chi2_end=list(self.chi2_end), iterations=list(self.iterations),
                 trials=list(self.trials))
        return d


class LocalBAProblem(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_poses", "n_local", "n_points", "n_edges", "nlevels")] + \
               [(k, C.c_void_p) for k in ("Tcw", "fixed", "cam", "inv_level_sigma2", "world_pos", "edge_point", "edge_pose",
                                          "edge_octave", "edge_xy", "edge_u_right", "d_stop", "d_Tcw_d", "d_Tcw", "d_pos_d",
                                          "d_pos", "d_erase", "d_result")]


LBA_MAX_POSES, LBA_MAX_FREE, LBA_MAX_POINTS, LBA_MAX_EDGES = 1024, 96, 16384, 262144


class BundleAdjustmentResult(C.Structure):
    _fields_ = [("chi2_start", C.c_double), ("chi2_end", C.c_double)] + \
               [(k, C.c_int32) for k in ("n_edges", "iterations", "trials", "stopped", "n_bad_index", "n_not_included",
                                         "reduced_in_lds", "pad_")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class BundleAdjustmentProblem(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_poses", "n_points", "n_edges", "nlevels", "n_iterations", "robust")] + \
               [(k, C.c_void_p) for k in ("Tcw", "fixed", "cam", "inv_level_sigma2", "world_pos", "edge_point", "edge_pose",
                                          "edge_octave", "edge_xy", "edge_u_right", "d_stop", "d_Tcw_d", "d_Tcw", "d_pos_d",
                                          "d_pos", "d_not_included", "d_result")]


BA_MAX_POSES, BA_MAX_FREE, BA_MAX_POINTS, BA_MAX_EDGES, BA_MAX_ITERATIONS = 1024, 256, 65536, 1 << 20, 100


class EssentialGraphResult(C.Structure):
    _fields_ = [("chi2_start", C.c_double), ("chi2_end", C.c_double)] + \
               [(k, C.c_int32) for k in ("iterations", "trials", "stopped", "n_edges", "n_bad_index", "n_free_active",
                                         "envelope", "bandwidth", "n_bad_ref", "pad_")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class EssentialGraphProblem(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_vertices", "n_edges", "n_iterations", "fix_scale")] + \
               [(k, C.c_void_p) for k in ("Scw", "Snc", "fixed", "edge_i", "edge_j", "edge_kind", "d_stop", "d_Siw_d", "d_Tiw",
                                          "d_result")]


EG_MAX_VERTICES, EG_MAX_EDGES, EG_MAX_POINTS, EG_MAX_ENVELOPE, EG_MAX_ITERATIONS = 8192, 1 << 18, 1 << 22, 1 << 26, 100


class Sim3Result(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n", "max_its", "n_bad_index", "n_bad_triple", "accepted", "n_inliers",
                                         "best_inliers", "best_iteration", "iterations", "no_more")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Sim3Problem(C.Structure):
    _fields_ = [("n1", C.c_int32), ("n_hyp", C.c_int32), ("valid", C.c_void_p), ("Xw1", C.c_void_p), ("Xw2", C.c_void_p),
                ("octave1", C.c_void_p), ("octave2", C.c_void_p), ("triples", C.c_void_p), ("T1w", C.c_float * 16),
                ("T2w", C.c_float * 16), ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float),
                ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float),
                ("level_sigma2", C.c_float * MAX_LEVELS), ("nlevels", C.c_int32), ("fix_scale", C.c_int32),
                ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("probability", C.c_double),
                ("start_iteration", C.c_int32), ("best_so_far", C.c_int32), ("counts", C.c_void_p), ("R", C.c_void_p),
                ("t", C.c_void_p), ("s", C.c_void_p), ("T12", C.c_void_p), ("masks", C.c_void_p), ("indices1", C.c_void_p),
                ("result", C.c_void_p)]


class Sim3OptResult(C.Structure):
    _fields_ = [("R12_d", C.c_double * 9), ("t12_d", C.c_double * 3), ("s12_d", C.c_double), ("R12", C.c_float * 9),
                ("t12", C.c_float * 3), ("s12", C.c_float), ("T12", C.c_float * 16), ("Scw", C.c_float * 16)] + \
               [(k, C.c_int32) for k in ("n_correspondences", "n_bad", "n_inliers", "stages", "iterations", "trials",
                                         "n_bad_index")]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_[8:]}
        d.update(R12_d=np.array(self.R12_d, np.float64).reshape(3, 3), t12_d=np.array(self.t12_d, np.float64),
                 s12_d=np.float64(self.s12_d), R12=np.array(self.R12, np.float32).reshape(3, 3),
                 t12=np.array(self.t12, np.float32), s12=np.float32(self.s12),
                 T12=np.array(self.T12, np.float32).reshape(4, 4), Scw=np.array(self.Scw, np.float32).reshape(4, 4))
        return d


class Sim3OptProblem(C.Structure):
    _fields_ = [("n1", C.c_int32), ("nlevels", C.c_int32), ("valid", C.c_void_p), ("Xw1", C.c_void_p), ("Xw2", C.c_void_p),
                ("octave1", C.c_void_p), ("octave2", C.c_void_p), ("kp1_xy", C.c_void_p), ("kp2_xy", C.c_void_p),
                ("T1w", C.c_float * 16), ("T2w", C.c_float * 16), ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float),
                ("cy1", C.c_float), ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float),
                ("inv_level_sigma2", C.c_float * MAX_LEVELS), ("R12", C.c_float * 9), ("t12", C.c_float * 3),
                ("s12", C.c_float), ("th2", C.c_float), ("fix_scale", C.c_int32), ("pad_", C.c_int32),
                ("inlier", C.c_void_p), ("result", C.c_void_p)]


class PnpResult(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n", "min_inliers", "max_its", "n_bad_index", "n_bad_set", "accepted", "n_inliers",
                                         "best_inliers", "best_iteration", "iterations", "no_more", "pad_")] + \
               [("Tcw", C.c_float * 16)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_[:11]}
        d["Tcw"] = np.array(self.Tcw, np.float32).reshape(4, 4)
        return d


class PnpProblem(C.Structure):
    _fields_ = [("n1", C.c_int32), ("n_hyp", C.c_int32), ("valid", C.c_void_p), ("Xw", C.c_void_p), ("kp", C.c_void_p),
                ("octave", C.c_void_p), ("sets", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("level_sigma2", C.c_float * MAX_LEVELS), ("nlevels", C.c_int32), ("min_set", C.c_int32),
                ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("epsilon", C.c_float), ("th2", C.c_float),
                ("probability", C.c_double), ("start_iteration", C.c_int32), ("best_so_far", C.c_int32),
                ("n_iterations", C.c_int32), ("pad_", C.c_int32), ("counts", C.c_void_p), ("Tcw", C.c_void_p),
                ("masks", C.c_void_p), ("refined_mask", C.c_void_p), ("indices", C.c_void_p), ("result", C.c_void_p)]


class InitResult(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_bad_index", C.c_int32), ("n_bad_set", C.c_int32), ("best_h", C.c_int32),
                ("best_f", C.c_int32), ("SH", C.c_float), ("SF", C.c_float), ("RH", C.c_float), ("used_homography", C.c_int32),
                ("n_inliers", C.c_int32), ("n_good", C.c_int32 * 8), ("cos_parallax", C.c_float * 8), ("best_motion", C.c_int32),
                ("second_best_good", C.c_int32), ("success", C.c_int32), ("parallax_deg", C.c_float), ("H21", C.c_float * 9),
                ("F21", C.c_float * 9), ("R21", C.c_float * 9), ("t21", C.c_float * 3)]

    def as_dict(self):
        d = {}
        for k, t in self._fields_:
            v = getattr(self, k)
            if k in ("n_good", "cos_parallax", "t21"):
                d[k] = np.array(v, np.int32 if k == "n_good" else np.float32)
            elif k in ("H21", "F21", "R21"):
                d[k] = np.array(v, np.float32).reshape(3, 3)
            else:
                d[k] = np.float32(v) if t is C.c_float else v
        return d


class InitProblem(C.Structure):
    _fields_ = [("n1", C.c_int32), ("n2", C.c_int32), ("kp1", C.c_void_p), ("kp2", C.c_void_p), ("matches12", C.c_void_p),
                ("sets", C.c_void_p), ("n_hyp", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("sigma", C.c_float), ("min_parallax", C.c_float), ("min_triangulated", C.c_int32),
                ("scores_h", C.c_void_p), ("scores_f", C.c_void_p), ("masks_h", C.c_void_p), ("masks_f", C.c_void_p),
                ("R21", C.c_void_p), ("t21", C.c_void_p), ("P3D", C.c_void_p), ("triangulated", C.c_void_p),
                ("result", C.c_void_p)]


class NewPointsFrame(C.Structure):
    _fields_ = [("n", C.c_int32), ("nlevels", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("kp_x", "kp_y", "kp_octave", "kp_angle", "u_right", "desc", "has_mp", "node", "depth",
                                          "kp_raw", "cos_stereo")] + \
               [("Tcw", C.c_float * 16), ("Twc", C.c_float * 16)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mbf")] + \
               [("level_sigma2", C.c_float * MAX_LEVELS), ("scale_factors", C.c_float * MAX_LEVELS), ("F12", C.c_float * 9),
                ("ex", C.c_float), ("ey", C.c_float)]


class NewPointsProblem(C.Structure):
    _fields_ = [("kf1", NewPointsFrame), ("neighbours", C.c_void_p), ("nn", C.c_int32), ("only_stereo", C.c_int32),
                ("check_orientation", C.c_int32), ("ratio_factor", C.c_float)] + \
               [(k, C.c_void_p) for k in ("stop", "match12", "status", "x3d", "n_matches", "n_created", "n_done")]


NEW_POINTS_MAX_NEIGHBOURS = 32
(NP_NONE, NP_TRIANGULATED, NP_UNPROJECT1, NP_UNPROJECT2, NP_LOW_PARALLAX, NP_W_ZERO, NP_Z1, NP_Z2, NP_REPROJ1, NP_REPROJ2,
 NP_ZERO_DIST, NP_SCALE, NP_NON_FINITE, NP_STEREO_DEPTH, NP_BAD_OCTAVE) = (0, 1, 2, 3, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10, -11)


_LIB = None

# every symbol include/orbgpu.h declares (checked by tests/test_abi.py against the header text)
class CovisLocalMapResult(C.Structure):
    """orbgpu_covis_local_map_result"""
    _fields_ = [("ref_kf", C.c_int64), ("n_kfs", C.c_int32), ("n_points", C.c_int32), ("max_votes", C.c_int32),
                ("n_voted", C.c_int32), ("kept_previous", C.c_int32), ("n_unknown_previous", C.c_int32)]


class CovisCullingResult(C.Structure):
    """orbgpu_covis_culling_result"""
    _fields_ = [("n_culled", C.c_int32), ("n_to_be_erased", C.c_int32), ("n_skipped", C.c_int32), ("n_points_bad", C.c_int32),
                ("n_query_points", C.c_int32)]


class CovisRefreshResult(C.Structure):
    """orbgpu_covis_refresh_result"""
    _fields_ = [("n_descriptors", C.c_int32), ("n_normals", C.c_int32), ("n_no_obs", C.c_int32), ("n_overflow", C.c_int32),
                ("n_no_desc", C.c_int32), ("n_no_centre", C.c_int32), ("n_no_ref", C.c_int32), ("n_unknown", C.c_int32),
                ("n_bad", C.c_int32), ("max_obs", C.c_int32), ("n_entries", C.c_int64)]


class CompactResult(C.Structure):
    """orbgpu_compact_result"""
    _fields_ = [("compacted", C.c_int32), ("rows_before", C.c_int32), ("rows_after", C.c_int32), ("rows_bad_kept", C.c_int32),
                ("row_capacity", C.c_int32), ("slots_before", C.c_int64), ("slots_after", C.c_int64), ("slot_capacity", C.c_int64)]


def _compact_call(fn, h):
    res = CompactResult()
    check(fn(h, C.byref(res)))
    return {name: getattr(res, name) for name, _ in CompactResult._fields_}


REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH = 1, 2
REFRESH_NO_OBS, REFRESH_OVERFLOW, REFRESH_NO_DESC, REFRESH_NO_CENTRE = 0x01, 0x02, 0x04, 0x08
REFRESH_NO_REF, REFRESH_UNKNOWN, REFRESH_BAD = 0x10, 0x20, 0x40
COVIS_REFRESH_MAX_OBS = 1024


def _refresh_call(fn, head, ids, ref_kf_ids, mid, what, outputs, initial):
    """the shared tail of CovisibilityGraph.refresh_points and MapPointTable.refresh: the in/out arrays (copies of `initial`
    where given, zeros otherwise; None where `outputs` leaves them out), the call -- `head` before n, `mid` before `what` --
    and the result as a dict"""
    n = len(ids)
    ref = np.ascontiguousarray(ref_kf_ids, np.int64).reshape(-1)
    if len(ref) != n:
        raise ValueError("one reference key frame per map point")
    shapes = dict(normal=((n, 3), np.float32), min_dist=((n,), np.float32), max_dist=((n,), np.float32), desc=((n, 32), np.uint8),
                  desc_kf=((n,), np.int64), desc_idx=((n,), np.int32))
    out = {}
    for name, (shape, dt) in shapes.items():
        if name not in outputs:
            out[name] = None
        elif initial is not None and name in initial:
            out[name] = np.array(initial[name], dt).reshape(shape)
        else:
            out[name] = np.zeros(shape, dt)
    n_slots, status = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
    res = CovisRefreshResult()
    check(fn(*head, n, _p(ids), _p(ref), *mid, int(what), _p(out["normal"]), _p(out["min_dist"]), _p(out["max_dist"]), _p(out["desc"]),
             _p(out["desc_kf"]), _p(out["desc_idx"]), _p(n_slots), _p(status), C.byref(res)))
    out = {k: v for k, v in out.items() if v is not None}
    out.update(n_slots=n_slots[:n].copy(), status=status[:n].copy())
    out.update({name: getattr(res, name) for name, _ in CovisRefreshResult._fields_})
    return out


REFRESH_OUTPUTS = ("normal", "min_dist", "max_dist", "desc", "desc_kf", "desc_idx")

ABI_SYMBOLS = [
    "orbgpu_last_error_string", "orbgpu_abi_version", "orbgpu_device_count", "orbgpu_measure_copy_bandwidth",
    "orbgpu_set_trig_mode", "orbgpu_get_trig_mode", "orbgpu_trig_table_info", "orbgpu_trig_host_eval", "orbgpu_trig_eval",
    "orbgpu_extractor_create", "orbgpu_extractor_destroy", "orbgpu_extractor_get_levels",
    "orbgpu_extractor_get_scale_factor", "orbgpu_extractor_get_scale_factors",
    "orbgpu_extractor_get_inv_scale_factors", "orbgpu_extractor_get_sigma2", "orbgpu_extractor_get_inv_sigma2",
    "orbgpu_extractor_get_quotas", "orbgpu_extractor_max_keypoints", "orbgpu_extract", "orbgpu_extract_batch",
    "orbgpu_extract_batch_device", "orbgpu_extractor_get_pyramid_level", "orbgpu_extractor_debug_read",
    "orbgpu_extractor_graph_state", "orbgpu_extractor_debug_quadtree_config", "orbgpu_extractor_set_profiling", "orbgpu_extractor_set_concurrent_blur", "orbgpu_extractor_set_fast_early_out", "orbgpu_extractor_set_stage_signal", "orbgpu_extractor_stage_count", "orbgpu_extractor_stage_name",
    "orbgpu_extractor_stage_times",
    "orbgpu_pipeline_create", "orbgpu_pipeline_destroy", "orbgpu_pipeline_parts", "orbgpu_pipeline_part",
    "orbgpu_pipeline_extract_device", "orbgpu_pipeline_wait",
    "orbgpu_hamming256", "orbgpu_match_bf", "orbgpu_matcher_create", "orbgpu_matcher_destroy",
    "orbgpu_match_bf_batch_device", "orbgpu_matcher_last_sweeps", "orbgpu_matcher_last_launch",
    "orbgpu_assign_features_to_grid",
    "orbgpu_frame_glue_batch_device", "orbgpu_stereo_matches_batch_device", "orbgpu_compute_stereo_matches",
    "orbgpu_undistort_points", "orbgpu_search_local_points_device", "orbgpu_search_local_points_batch_device", "orbgpu_search_by_projection_last_device", "orbgpu_projection_last_sweeps", "orbgpu_distinctive_descriptors", "orbgpu_search_by_projection_sim3",
    "orbgpu_search_by_projection", "orbgpu_search_by_projection_last", "orbgpu_search_by_projection_keyframe",
    "orbgpu_mappoint_table_create", "orbgpu_mappoint_table_destroy", "orbgpu_mappoint_table_rows",
    "orbgpu_mappoint_table_upsert", "orbgpu_mappoint_table_set_bad", "orbgpu_mappoint_table_set_observations",
    "orbgpu_mappoint_table_read", "orbgpu_mappoint_table_last_unknown", "orbgpu_mappoint_table_retain", "orbgpu_frame_create", "orbgpu_frame_destroy", "orbgpu_frame_upload",
    "orbgpu_frame_device_view", "orbgpu_search_local_points_table", "orbgpu_search_by_projection_last_table",
    "orbgpu_pose_optimization", "orbgpu_pose_optimization_device", "orbgpu_pose_optimization_batch_device",
    "orbgpu_pose_optimization_table", "orbgpu_pose_last_spills",
    "orbgpu_local_ba", "orbgpu_local_ba_device", "orbgpu_local_ba_batch_device", "orbgpu_local_ba_last_spills",
    "orbgpu_bundle_adjustment", "orbgpu_bundle_adjustment_device", "orbgpu_bundle_adjustment_batch_device",
    "orbgpu_bundle_adjustment_last_spills",
    "orbgpu_essential_graph", "orbgpu_essential_graph_device", "orbgpu_essential_graph_batch_device",
    "orbgpu_essential_graph_correct_points_device", "orbgpu_sim3_from_pose",
    "orbgpu_sim3_ransac_iterations", "orbgpu_sim3_solve_device", "orbgpu_sim3_solve_batch_device", "orbgpu_sim3_solve",
    "orbgpu_sim3_solve_all",
    "orbgpu_sim3_optimize", "orbgpu_sim3_optimize_device", "orbgpu_sim3_optimize_batch_device",
    "orbgpu_sim3_opt_last_spills",
    "orbgpu_pnp_ransac_parameters", "orbgpu_pnp_solve_device", "orbgpu_pnp_solve_batch_device", "orbgpu_pnp_solve",
    "orbgpu_pnp_solve_all", "orbgpu_pnp_solve_table",
    "orbgpu_initializer_cos_limits", "orbgpu_initializer_device", "orbgpu_initializer_batch_device", "orbgpu_initializer",
    "orbgpu_initializer_all",
    "orbgpu_create_new_map_points_device", "orbgpu_create_new_map_points",
    "orbgpu_keyframe_db_create", "orbgpu_keyframe_db_destroy", "orbgpu_keyframe_db_clear", "orbgpu_keyframe_db_size",
    "orbgpu_keyframe_db_add", "orbgpu_keyframe_db_erase", "orbgpu_keyframe_db_set_covisibles", "orbgpu_keyframe_db_score",
    "orbgpu_keyframe_db_detect_loop", "orbgpu_keyframe_db_detect_reloc", "orbgpu_keyframe_db_last_query",
    "orbgpu_keyframe_db_debug_global_queries", "orbgpu_keyframe_db_compact",
    "orbgpu_covis_graph_create", "orbgpu_covis_graph_destroy", "orbgpu_covis_graph_clear", "orbgpu_covis_graph_size",
    "orbgpu_covis_graph_add_keyframe", "orbgpu_covis_graph_set_slots", "orbgpu_covis_graph_set_bad",
    "orbgpu_covis_graph_set_parent", "orbgpu_covis_graph_set_covisibles", "orbgpu_covis_local_map",
    "orbgpu_covis_connections", "orbgpu_covis_graph_debug_global_queries", "orbgpu_covis_graph_compact",
    "orbgpu_covis_graph_set_keypoints", "orbgpu_covis_observations", "orbgpu_covis_keyframe_culling",
    "orbgpu_covis_graph_set_scale_factors", "orbgpu_covis_graph_set_descriptors", "orbgpu_covis_graph_set_centres",
    "orbgpu_covis_refresh_points", "orbgpu_mappoint_table_refresh",
    "orbgpu_vocabulary_create", "orbgpu_vocabulary_destroy", "orbgpu_vocabulary_size", "orbgpu_bow_transform",
    "orbgpu_bow_transform_batch_device", "orbgpu_search_by_bow", "orbgpu_search_by_bow_batch_device",
    "orbgpu_search_by_bow_keyframes", "orbgpu_search_for_triangulation", "orbgpu_search_for_initialization", "orbgpu_fuse", "orbgpu_fuse_sim3",
    "orbgpu_search_by_sim3",
    "orbgpu_mappoint_record_bytes", "orbgpu_write_mappoint_record", "orbgpu_keyframe_record_bytes",
    "orbgpu_write_keyframe_record", "orbgpu_pcd_binary_header", "orbgpu_write_pcd_binary", "orbgpu_cloud_save_pcd",
    "orbgpu_cloud_create", "orbgpu_cloud_destroy", "orbgpu_cloud_insert", "orbgpu_cloud_insert_device",
    "orbgpu_cloud_clear", "orbgpu_cloud_append_filtered", "orbgpu_cloud_last_path", "orbgpu_cloud_set_profiling", "orbgpu_cloud_last_insert_ms", "orbgpu_cloud_rebuild",
    "orbgpu_cloud_size", "orbgpu_cloud_download", "orbgpu_cloud_last_overflow", "orbgpu_backproject",
    "orbgpu_voxel_filter", "orbgpu_cloud_remove_outliers", "orbgpu_statistical_outlier_removal",
]


def lib():
    """Loads liborbgpu.so. Raises OSError if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if "torch" not in sys.modules:
        # torch wheels bundle their own HIP runtime; if liborbgpu.so pulls in /opt/rocm's copy first,
        # a later `import torch` in the same process cannot see the GPU ("No HIP GPUs are available").
        # Loading torch first makes both share one runtime.  Pure plumbing: nothing here uses torch.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(LIB_PATH):
        raise OSError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(the HIP extension is the product; there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, f32, sz = C.c_void_p, C.c_int32, C.c_float, C.c_size_t
    L.orbgpu_last_error_string.restype = C.c_char_p
    L.orbgpu_extractor_stage_name.restype = C.c_char_p
    L.orbgpu_extractor_stage_name.argtypes = [i32]
    sigs = {
        "orbgpu_extractor_create": [vp, vp],
        "orbgpu_set_trig_mode": [i32],
        "orbgpu_trig_table_info": [vp, vp],
        "orbgpu_extractor_destroy": [vp],
        "orbgpu_extractor_get_levels": [vp, vp],
        "orbgpu_extractor_get_scale_factor": [vp, vp],
        "orbgpu_extractor_get_scale_factors": [vp, vp],
        "orbgpu_extractor_get_inv_scale_factors": [vp, vp],
        "orbgpu_extractor_get_sigma2": [vp, vp],
        "orbgpu_extractor_get_inv_sigma2": [vp, vp],
        "orbgpu_extractor_get_quotas": [vp, vp],
        "orbgpu_extractor_max_keypoints": [vp, i32, i32, vp],
        "orbgpu_extract": [vp, vp, i32, i32, sz, vp, vp, i32, vp],
        "orbgpu_extract_batch": [vp, vp, i32, i32, i32, sz, sz, vp, vp, i32, vp],
        "orbgpu_extract_batch_device": [vp, vp, i32, i32, i32, sz, sz, vp, vp, i32, vp, vp],
        "orbgpu_extractor_get_pyramid_level": [vp, i32, i32, vp, sz, vp, vp],
        "orbgpu_extractor_debug_read": [vp, i32, i32, i32, vp, sz, vp, vp],
        "orbgpu_extractor_set_profiling": [vp, i32],
        "orbgpu_extractor_set_stage_signal": [vp, i32, vp],
        "orbgpu_extractor_stage_times": [vp, vp],
        "orbgpu_pipeline_create": [vp, i32, vp],
        "orbgpu_pipeline_destroy": [vp],
        "orbgpu_pipeline_parts": [vp, vp],
        "orbgpu_pipeline_part": [vp, i32, vp],
        "orbgpu_pipeline_extract_device": [vp, vp, i32, i32, i32, sz, sz, vp, vp, i32, vp, vp, vp],
        "orbgpu_pipeline_wait": [vp, vp],
        "orbgpu_hamming256": [vp, vp, i32, vp, i32],
        "orbgpu_match_bf": [vp, vp, vp, i32, vp, vp, i32, i32, f32, i32, vp, vp, i32],
        "orbgpu_matcher_create": [i32, i32, i32, vp],
        "orbgpu_matcher_destroy": [vp],
        "orbgpu_match_bf_batch_device": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, sz, i32, f32, i32, vp, vp, vp],
        "orbgpu_matcher_last_sweeps": [vp, vp],
        "orbgpu_matcher_last_launch": [vp, vp, vp, vp],
        "orbgpu_search_by_bow_batch_device": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, i32, f32, i32, vp, vp,
                                              vp],
        "orbgpu_assign_features_to_grid": [i32, vp, vp, f32, f32, f32, f32, vp, vp],
        "orbgpu_frame_glue_batch_device": [i32, i32, i32, vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp, vp],
        "orbgpu_stereo_matches_batch_device": [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, f32, vp, vp, vp,
                                               vp],
        "orbgpu_compute_stereo_matches": [vp, vp, i32, vp, vp, i32, vp, vp, f32, f32, vp, vp],
        "orbgpu_undistort_points": [i32, vp, vp, vp, i32],
        "orbgpu_search_local_points_device": [vp, vp, vp, f32, f32, f32, f32, f32, f32, f32, f32, f32, vp, vp, vp, i32, vp],
        "orbgpu_projection_last_sweeps": [vp, vp],
        "orbgpu_distinctive_descriptors": [i32, vp, vp, vp, i32],
        "orbgpu_search_by_projection_sim3": [vp, vp, f32, f32, f32, f32, f32, vp, i32, vp, vp, i32],
        "orbgpu_search_by_projection": [vp, vp, f32, f32, vp, vp, i32],
        "orbgpu_search_by_projection_last": [vp, vp, f32, f32, f32, f32, f32, f32, vp, f32, i32, i32, vp, vp, i32],
        "orbgpu_search_by_projection_keyframe": [vp, vp, f32, f32, f32, f32, f32, vp, f32, i32, i32, vp, vp, i32],
        "orbgpu_cloud_create": [C.c_double, i32, vp],
        "orbgpu_cloud_destroy": [vp],
        "orbgpu_cloud_insert": [vp, vp, sz, vp, sz, i32, i32, f32, f32, f32, f32, vp],
        "orbgpu_cloud_insert_device": [vp, vp, sz, vp, sz, i32, i32, f32, f32, f32, f32, vp],
        "orbgpu_cloud_last_path": [vp, vp],
        "orbgpu_cloud_set_profiling": [vp, i32],
        "orbgpu_cloud_last_insert_ms": [vp, vp],
        "orbgpu_cloud_rebuild": [vp, i32, vp, sz, vp, sz, i32, i32, f32, f32, f32, f32, vp],
        "orbgpu_cloud_size": [vp, vp],
        "orbgpu_cloud_download": [vp, vp, C.c_int64, vp],
        "orbgpu_cloud_last_overflow": [vp, vp],
        "orbgpu_backproject": [vp, sz, vp, sz, i32, i32, f32, f32, f32, f32, vp, vp, C.c_int64, vp, i32],
        "orbgpu_voxel_filter": [vp, C.c_int64, C.c_double, vp, C.c_int64, vp, vp, i32],
        "orbgpu_cloud_remove_outliers": [vp, i32, C.c_double, vp],
        "orbgpu_statistical_outlier_removal": [vp, C.c_int64, i32, C.c_double, vp, C.c_int64, vp, vp, i32],
        "orbgpu_keyframe_db_create": [i32, i32, i32, i32, vp],
        "orbgpu_keyframe_db_destroy": [vp],
        "orbgpu_keyframe_db_clear": [vp],
        "orbgpu_keyframe_db_size": [vp, vp],
        "orbgpu_keyframe_db_add": [vp, C.c_int64, i32, vp, vp],
        "orbgpu_keyframe_db_erase": [vp, i32, vp, vp],
        "orbgpu_keyframe_db_set_covisibles": [vp, C.c_int64, i32, vp],
        "orbgpu_keyframe_db_score": [vp, i32, vp, vp, i32, vp, vp],
        "orbgpu_keyframe_db_detect_loop": [vp, i32, vp, vp, i32, vp, f32, i32, vp, vp],
        "orbgpu_keyframe_db_detect_reloc": [vp, i32, vp, vp, i32, vp, vp],
        "orbgpu_keyframe_db_last_query": [vp, i32, vp, vp, vp, vp, vp, vp, vp],
        "orbgpu_keyframe_db_debug_global_queries": [vp, vp],
        "orbgpu_keyframe_db_compact": [vp, vp],
        "orbgpu_covis_graph_create": [i32, i32, C.c_int64, vp],
        "orbgpu_covis_graph_destroy": [vp],
        "orbgpu_covis_graph_clear": [vp],
        "orbgpu_covis_graph_size": [vp, vp, vp],
        "orbgpu_covis_graph_add_keyframe": [vp, C.c_int64, i32, vp],
        "orbgpu_covis_graph_set_slots": [vp, i32, vp, vp, vp, vp],
        "orbgpu_covis_graph_set_bad": [vp, i32, vp, vp],
        "orbgpu_covis_graph_set_parent": [vp, C.c_int64, C.c_int64],
        "orbgpu_covis_graph_set_covisibles": [vp, C.c_int64, i32, vp],
        "orbgpu_covis_local_map": [vp, i32, vp, i32, vp, i32, vp, i32, vp, vp],
        "orbgpu_covis_connections": [vp, C.c_int64, i32, i32, vp, vp, vp, i32, vp, vp, vp],
        "orbgpu_covis_graph_debug_global_queries": [vp, vp],
        "orbgpu_covis_graph_compact": [vp, vp],
        "orbgpu_covis_graph_set_keypoints": [vp, C.c_int64, i32, vp],
        "orbgpu_covis_observations": [vp, i32, vp, vp, vp],
        "orbgpu_covis_keyframe_culling": [vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp],
        "orbgpu_covis_graph_set_scale_factors": [vp, i32, vp],
        "orbgpu_covis_graph_set_descriptors": [vp, C.c_int64, i32, vp],
        "orbgpu_covis_graph_set_centres": [vp, i32, vp, vp, vp],
        "orbgpu_covis_refresh_points": [vp, i32, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "orbgpu_mappoint_table_refresh": [vp, vp, i32, vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    }
    for name, args in sigs.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.argtypes = args
            fn.restype = C.c_int
    _LIB = L
    return L


def check(status):
    if status != OK:
        raise OrbGpuError(status, lib().orbgpu_last_error_string().decode("utf-8", "replace"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# What the solver and optimiser families (pose_optimization, sim3_solve, sim3_optimize, pnp_solve, initializer) share: the two device
# flavours' calls, and the setters of their *_problem builders.
def _batch_device(family, cls, make, problems, stream, device_id):
    """orbgpu_<family>_batch_device over make(p), a cls structure, of every problem."""
    arr = (cls * max(len(problems), 1))(*[make(p) for p in problems])
    fn = getattr(lib(), "orbgpu_%s_batch_device" % family)
    fn.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    check(fn(len(problems), arr, device_id, stream))


def _one_device(family, q, stream, device_id):
    """orbgpu_<family>_device over the problem structure q."""
    fn = getattr(lib(), "orbgpu_%s_device" % family)
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    check(fn(C.byref(q), device_id, stream))


def _set_pointers(q, p, names):
    for k in names:
        setattr(q, k, p.get(k) or None)


def _set_floats(field, a):
    """A float array field of a structure (4x4, 3x3, a vector) from anything of that many elements."""
    field[:] = np.asarray(a, np.float32).reshape(len(field)).tolist()


def _set_intrinsics(q, K, suffix=""):
    fx, fy, cx, cy = (float(k) for k in K)
    for name, v in (("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy)):
        setattr(q, name + suffix, v)


def _set_levels(q, p, field):
    """q.<field>[l] per pyramid level from p[field]; nlevels from p, by default the array's length."""
    sg = np.asarray(p[field], np.float32)
    q.nlevels = int(p.get("nlevels", len(sg)))
    for l in range(min(len(sg), MAX_LEVELS)):
        getattr(q, field)[l] = float(sg[l])


def device_count():
    return lib().orbgpu_device_count()


def measure_copy_bandwidth(nbytes=1 << 30, reps=10, device_id=0):
    """Achieved GB/s (read + write) of a plain device-to-device copy kernel: the practical HBM roofline."""
    L = lib()
    L.orbgpu_measure_copy_bandwidth.argtypes = [C.c_size_t, C.c_int32, C.c_int32, C.c_void_p]
    v = C.c_float()
    check(L.orbgpu_measure_copy_bandwidth(nbytes, reps, device_id, C.byref(v)))
    return v.value


TRIG_HOST_LIBM, TRIG_ROUNDED_DOUBLE = 0, 1


def set_trig_mode(mode):
    """cos / sin of computeOrbDescriptor (ORBextractor.cc:112-113) for extractors created from now on: TRIG_HOST_LIBM
    (default: this host's cosf / sinf, bit for bit) or TRIG_ROUNDED_DOUBLE ((float)cos((double)angle))."""
    check(lib().orbgpu_set_trig_mode(int(mode)))


def get_trig_mode():
    return lib().orbgpu_get_trig_mode()


def trig_table_info():
    """(entries of the host-libm exception table or -1 if it has not been built, milliseconds its scan took)."""
    n, ms = C.c_int64(), C.c_double()
    check(lib().orbgpu_trig_table_info(C.byref(n), C.byref(ms)))
    return n.value, ms.value


def trig_host_eval(x):
    """(cos, sin, from_table) of the float x as TRIG_HOST_LIBM delivers them; needs no device."""
    L = lib()
    L.orbgpu_trig_host_eval.argtypes = [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    c, s, t = C.c_float(), C.c_float(), C.c_int32()
    check(L.orbgpu_trig_host_eval(float(x), C.byref(c), C.byref(s), C.byref(t)))
    return np.float32(c.value), np.float32(s.value), t.value


def trig_eval(x, device_id=0):
    """cos / sin of the float32 array x as the DEVICE computes them for the descriptor stage (current trig mode)."""
    L = lib()
    L.orbgpu_trig_eval.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    x = np.ascontiguousarray(x, np.float32)
    c, s = np.zeros(len(x), np.float32), np.zeros(len(x), np.float32)
    check(L.orbgpu_trig_eval(_p(x), len(x), _p(c), _p(s), device_id))
    return c, s


# --------------------------------------------------------------------------------------------
# ORBextractor (reference include/ORBextractor.h:46-110)
# --------------------------------------------------------------------------------------------
class ORBextractor:
    """Mirror of ORB_SLAM2::ORBextractor; __call__ mirrors operator() (ORBextractor.h:59-61)."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, device_id=0,
                 max_batch=1):
        self.L = lib()
        self.params = ExtractorParams(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device_id, max_batch)
        h = C.c_void_p()
        check(self.L.orbgpu_extractor_create(C.byref(self.params), C.byref(h)))
        self.h = h
        self.nfeatures, self.nlevels = nfeatures, nlevels

    def close(self):
        if getattr(self, "h", None):
            self.L.orbgpu_extractor_destroy(self.h)
            self.h = None

    __del__ = close

    def GetLevels(self):
        n = C.c_int32()
        check(self.L.orbgpu_extractor_get_levels(self.h, C.byref(n)))
        return n.value

    def GetScaleFactor(self):
        s = C.c_float()
        check(self.L.orbgpu_extractor_get_scale_factor(self.h, C.byref(s)))
        return s.value

    def _vec(self, fn, dtype):
        out = np.zeros(self.nlevels, dtype)
        check(fn(self.h, _p(out)))
        return out

    def GetScaleFactors(self):
        return self._vec(self.L.orbgpu_extractor_get_scale_factors, np.float32)

    def GetInverseScaleFactors(self):
        return self._vec(self.L.orbgpu_extractor_get_inv_scale_factors, np.float32)

    def GetScaleSigmaSquares(self):
        return self._vec(self.L.orbgpu_extractor_get_sigma2, np.float32)

    def GetInverseScaleSigmaSquares(self):
        return self._vec(self.L.orbgpu_extractor_get_inv_sigma2, np.float32)

    def quotas(self):
        return self._vec(self.L.orbgpu_extractor_get_quotas, np.int32)

    def max_keypoints(self, width, height):
        cap = C.c_int32()
        check(self.L.orbgpu_extractor_max_keypoints(self.h, width, height, C.byref(cap)))
        return cap.value

    def __call__(self, image, mask=None):
        """(keypoints, descriptors) of one 8-bit gray image; mask is ignored as in the reference."""
        k, d = self.extract_batch(np.asarray(image)[None])
        return k[0], d[0]

    def extract_batch(self, images):
        images = np.ascontiguousarray(images, np.uint8)
        if images.ndim != 3:
            raise ValueError("images must be [batch, h, w] uint8")
        b, h, w = images.shape
        if h == 0 or w == 0:
            return [np.zeros(0, KEYPOINT_DTYPE)] * b, [np.zeros((0, 32), np.uint8)] * b
        cap = self.max_keypoints(w, h)
        kps = np.zeros((b, cap), KEYPOINT_DTYPE)
        desc = np.zeros((b, cap, 32), np.uint8)
        n = np.zeros(b, np.int32)
        check(self.L.orbgpu_extract_batch(self.h, _p(images), b, w, h, images.strides[1], images.strides[0], _p(kps),
                                          _p(desc), cap, _p(n)))
        return [kps[i, :n[i]].copy() for i in range(b)], [desc[i, :n[i]].copy() for i in range(b)]

    def extract_batch_device(self, d_gray_ptr, batch, width, height, stride, frame_stride, d_kps_ptr, d_desc_ptr, cap,
                             d_nout_ptr, stream=0):
        check(self.L.orbgpu_extract_batch_device(self.h, d_gray_ptr, batch, width, height, stride, frame_stride,
                                                 d_kps_ptr, d_desc_ptr, cap, d_nout_ptr, stream))

    def pyramid_level(self, frame, level):
        """mvImagePyramid[level] of `frame` of the last call (ORBextractor.h:85)."""
        raw, pitch = self.debug_read(DBG_PYRAMID_PADDED, frame, level)
        img = raw.reshape(-1, pitch)
        return img

    def debug_read(self, what, frame, level):
        cap = 64 << 20
        buf = np.zeros(cap, np.uint8)
        n = C.c_size_t()
        aux = C.c_int32()
        check(self.L.orbgpu_extractor_debug_read(self.h, what, frame, level, _p(buf), cap, C.byref(n), C.byref(aux)))
        if what in (DBG_PYRAMID_PADDED, DBG_BLURRED_PADDED):
            return buf[:n.value].copy(), aux.value
        return buf[:n.value * 12].view(np.int32).reshape(-1, 3).copy(), 0

    def graph_counts(self):
        """(graphs recorded, graph replays) of the host entry points on this handle since its creation."""
        c = np.zeros(2, np.int32)
        n = C.c_size_t()
        check(self.L.orbgpu_extractor_debug_read(self.h, DBG_GRAPH_COUNTS, 0, 0, _p(c), c.nbytes, C.byref(n), None))
        return int(c[0]), int(c[1])

    def graph_state(self):
        v = C.c_int32()
        self.L.orbgpu_extractor_graph_state.argtypes = [C.c_void_p, C.c_void_p]
        check(self.L.orbgpu_extractor_graph_state(self.h, C.byref(v)))
        return v.value

    def quadtree_config(self, batch=1):
        """(keys of a level kept in LDS, threads per workgroup, dynamic LDS bytes) of k_quadtree for `batch` frames."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self.L.orbgpu_extractor_debug_quadtree_config.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        check(self.L.orbgpu_extractor_debug_quadtree_config(self.h, batch, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_concurrent_blur(self, on):
        check(self.L.orbgpu_extractor_set_concurrent_blur(self.h, int(on)))

    def get_pyramid_level(self, frame, level):
        """mvImagePyramid[level] of frame `frame` of the last call (ORBextractor.h:85) through the drop-in getter
        orbgpu_extractor_get_pyramid_level: (pixels HxW, width, height)."""
        buf = np.zeros((4112, 4112), np.uint8)  # the largest level the library accepts
        w, h = C.c_int32(), C.c_int32()
        check(self.L.orbgpu_extractor_get_pyramid_level(self.h, int(frame), int(level), _p(buf), buf.strides[0], C.byref(w),
                                                        C.byref(h)))
        return buf[:h.value, :w.value].copy(), w.value, h.value

    def set_fast_early_out(self, on):
        """Exact wave-level early-out of the FAST score network (orbgpu_extractor_set_fast_early_out)."""
        self.L.orbgpu_extractor_set_fast_early_out.argtypes = [C.c_void_p, C.c_int32]
        check(self.L.orbgpu_extractor_set_fast_early_out(self.h, int(on)))

    def set_profiling(self, on):
        check(self.L.orbgpu_extractor_set_profiling(self.h, int(on)))

    def set_stage_signal(self, stage_name, hip_event):
        """hip_event (raw hipEvent_t handle or None) is recorded after the named stage of every later device-batch call."""
        names = [self.L.orbgpu_extractor_stage_name(i).decode() for i in range(self.L.orbgpu_extractor_stage_count())]
        check(self.L.orbgpu_extractor_set_stage_signal(self.h, names.index(stage_name), C.c_void_p(hip_event or 0)))

    def stage_times(self):
        n = self.L.orbgpu_extractor_stage_count()
        ms = np.zeros(n, np.float32)
        check(self.L.orbgpu_extractor_stage_times(self.h, _p(ms)))
        return {self.L.orbgpu_extractor_stage_name(i).decode(): float(ms[i]) for i in range(n)}


class _PipelinePart(ORBextractor):
    """View of one part's handle (set_profiling / stage_times / set_stage_signal / debug reads); the pipeline owns it."""

    def __init__(self, L, h, nfeatures, nlevels):
        self.L, self.h, self.nfeatures, self.nlevels = L, h, nfeatures, nlevels

    def close(self):
        self.h = None

    __del__ = close


class ExtractorPipeline:
    """orbgpu_pipeline: a resident batch extracted as `parts` staggered sub-batches on streams of their own (include/orbgpu.h).
    Calls only enqueue; order consumers with done_event / wait(stream)."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, device_id=0, max_batch=1,
                 parts=2):
        self.L = lib()
        self.params = ExtractorParams(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device_id, max_batch)
        h = C.c_void_p()
        check(self.L.orbgpu_pipeline_create(C.byref(self.params), parts, C.byref(h)))
        self.h = h
        self.parts = []
        for k in range(parts):
            ph = C.c_void_p()
            check(self.L.orbgpu_pipeline_part(self.h, k, C.byref(ph)))
            self.parts.append(_PipelinePart(self.L, ph, nfeatures, nlevels))

    def close(self):
        if getattr(self, "h", None):
            for e in self.parts:
                e.h = None
            self.L.orbgpu_pipeline_destroy(self.h)
            self.h = None

    __del__ = close

    def max_keypoints(self, width, height):
        return self.parts[0].max_keypoints(width, height)

    def extract_batch_device(self, d_gray_ptr, batch, width, height, stride, frame_stride, d_kps_ptr, d_desc_ptr, cap,
                             d_nout_ptr, wait_event=None, done_event=None):
        check(self.L.orbgpu_pipeline_extract_device(self.h, d_gray_ptr, batch, width, height, stride, frame_stride, d_kps_ptr,
                                                    d_desc_ptr, cap, d_nout_ptr, C.c_void_p(wait_event or 0),
                                                    C.c_void_p(done_event or 0)))

    def wait(self, stream=0):
        check(self.L.orbgpu_pipeline_wait(self.h, C.c_void_p(stream or 0)))


# --------------------------------------------------------------------------------------------
# ORBmatcher (reference include/ORBmatcher.h:41-106)
# --------------------------------------------------------------------------------------------
def assign_features_to_grid(kp_x, kp_y, min_x, min_y, inv_w, inv_h):
    kp_x = np.ascontiguousarray(kp_x, np.float32)
    kp_y = np.ascontiguousarray(kp_y, np.float32)
    cs = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int32)
    items = np.zeros(max(1, len(kp_x)), np.int32)
    check(lib().orbgpu_assign_features_to_grid(len(kp_x), _p(kp_x), _p(kp_y), min_x, min_y, inv_w, inv_h, _p(cs),
                                               _p(items)))
    return cs, items[:cs[-1]].copy()


def make_camera(fx, fy, cx, cy, mbf, width, height, dist=(), device_id=0):
    """orbgpu_camera with the image bounds of Frame::ComputeImageBounds (Frame.cc:436-468)."""
    cam = Camera()
    cam.fx, cam.fy, cam.cx, cam.cy, cam.mbf = fx, fy, cx, cy, mbf
    for i in range(5):
        cam.dist[i] = float(dist[i]) if i < len(dist) else 0.0
    cam.min_x, cam.max_x, cam.min_y, cam.max_y = 0.0, float(width), 0.0, float(height)
    if cam.dist[0] != 0.0:
        c = undistort_points(np.array([[0, 0], [width, 0], [0, height], [width, height]], np.float32), cam, device_id)
        cam.min_x, cam.max_x = min(c[0, 0], c[2, 0]), max(c[1, 0], c[3, 0])
        cam.min_y, cam.max_y = min(c[0, 1], c[1, 1]), max(c[2, 1], c[3, 1])
    return cam


def undistort_points(xy, cam, device_id=0):
    """cv::undistortPoints(xy, xy, mK, mDistCoef, Mat(), mK) (orbgpu_undistort_points)."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.zeros_like(xy)
    check(lib().orbgpu_undistort_points(len(xy), _p(xy), C.byref(cam), _p(out), device_id))
    return out


def frame_glue_batch_device(batch, cap, d_kps, d_n, d_depth, depth_stride, depth_frame_stride, cam, d_kps_un,
                            d_u_right, d_kp_depth, d_cell_start, d_cell_items, stream=0, device_id=0):
    """UndistortKeyPoints + ComputeStereoFromRGBD + AssignFeaturesToGrid on the device
    (orbgpu_frame_glue_batch_device). cam: Camera (make_camera)."""
    check(lib().orbgpu_frame_glue_batch_device(device_id, batch, cap, d_kps, d_n, d_depth, depth_stride,
                                               depth_frame_stride, C.byref(cam), d_kps_un, d_u_right, d_kp_depth,
                                               d_cell_start, d_cell_items, stream))


def compute_stereo_matches(left, right, kps_l, desc_l, kps_r, desc_r, mbf, fx):
    """Frame::ComputeStereoMatches (Frame.cc:466-638) for frame 0 of the last calls of two ORBextractor handles (`left`
    may be `right`): (mvuRight, mvDepth) as float32 arrays of len(kps_l), -1 where there is no match
    (orbgpu_compute_stereo_matches)."""
    kl = np.ascontiguousarray(kps_l, KEYPOINT_DTYPE)
    kr = np.ascontiguousarray(kps_r, KEYPOINT_DTYPE)
    dl = np.ascontiguousarray(desc_l, np.uint8).reshape(-1, 32)
    dr = np.ascontiguousarray(desc_r, np.uint8).reshape(-1, 32)
    if len(dl) != len(kl) or len(dr) != len(kr):
        raise ValueError("key points and descriptors differ in count")
    u = np.zeros(len(kl), np.float32)
    d = np.zeros(len(kl), np.float32)
    check(lib().orbgpu_compute_stereo_matches(left.h, right.h, len(kl), _p(kl), _p(dl), len(kr), _p(kr), _p(dr),
                                              float(mbf), float(fx), _p(u), _p(d)))
    return u, d


def stereo_matches_batch_device(left, left_frame0, right, right_frame0, batch, cap, d_kps_l, d_n_l, d_desc_l, d_kps_r,
                                d_n_r, d_desc_r, mbf, fx, d_u_right, d_depth, d_n_stereo=None, stream=0):
    """Frame::ComputeStereoMatches for `batch` pairs of device-resident frames (orbgpu_stereo_matches_batch_device):
    pair p = frame left_frame0 + p of `left`'s last call and frame right_frame0 + p of `right`'s."""
    check(lib().orbgpu_stereo_matches_batch_device(left.h, left_frame0, right.h, right_frame0, batch, cap, d_kps_l, d_n_l,
                                                   d_desc_l, d_kps_r, d_n_r, d_desc_r, float(mbf), float(fx), d_u_right,
                                                   d_depth, d_n_stereo, stream))


def search_local_points_device(frame_view, table, Tcw, fx, fy, cx, cy, mbf, log_sf, th, nnratio, d_kp_to_mp, d_counts,
                               track=None, cos_limit=0.5, stream=0, device_id=0):
    """Tracking::SearchLocalPoints on device-resident data (orbgpu_search_local_points_device).
    frame_view: DeviceFrameView, table: DeviceMapPointTable, track: TrackScratch or None."""
    T = np.ascontiguousarray(Tcw, np.float32)
    check(lib().orbgpu_search_local_points_device(C.byref(frame_view), C.byref(table), _p(T), fx, fy, cx, cy, mbf, log_sf,
                                                  cos_limit, th, nnratio, d_kp_to_mp, d_counts,
                                                  C.byref(track) if track is not None else None, device_id, stream))


def search_local_points_batch_device(problems, cos_limit, th, nnratio, stream=0, device_id=0):
    """n independent Tracking::SearchLocalPoints problems in one call (orbgpu_search_local_points_batch_device).
    problems: list of dicts with frame (DeviceFrameView), table (DeviceMapPointTable), Tcw (4x4), fx, fy, cx, cy, mbf,
    log_sf, d_kp_to_mp, d_counts (device pointers) and optionally track (TrackScratch)."""
    n = len(problems)
    arr = (LocalPointsProblem * max(n, 1))()
    keep = []
    for k, p in enumerate(problems):
        T = np.ascontiguousarray(p["Tcw"], np.float32)
        keep.append(T)
        arr[k].frame = C.addressof(p["frame"])
        arr[k].table = C.addressof(p["table"])
        arr[k].Tcw = T.ctypes.data
        arr[k].fx, arr[k].fy, arr[k].cx, arr[k].cy, arr[k].mbf = p["fx"], p["fy"], p["cx"], p["cy"], p["mbf"]
        arr[k].log_scale_factor = p["log_sf"]
        track = p.get("track")  # optional TrackScratch of device arrays, as search_local_points_device takes it
        arr[k].d_kp_to_mp, arr[k].d_counts = p["d_kp_to_mp"], p["d_counts"]
        arr[k].d_track = C.addressof(track) if track is not None else None
    L = lib()
    L.orbgpu_search_local_points_batch_device.argtypes = [C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int32,
                                                          C.c_void_p]
    check(L.orbgpu_search_local_points_batch_device(n, arr, cos_limit, th, nnratio, device_id, stream))


def search_by_projection_last_device(cur_view, cur_Tcw, last_view, last_Tcw, fx, fy, cx, cy, mbf, mb, th, mono, check_ori,
                                     d_kp_to_mp, d_counts, stream=0, device_id=0):
    """TrackWithMotionModel's matcher on device-resident frames (orbgpu_search_by_projection_last_device).
    cur_view: DeviceFrameView, last_view: DeviceLastFrameView; poses are host 4x4 arrays."""
    Tc = np.ascontiguousarray(cur_Tcw, np.float32)
    Tl = np.ascontiguousarray(last_Tcw, np.float32)
    L = lib()
    L.orbgpu_search_by_projection_last_device.argtypes = [
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
        C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    check(L.orbgpu_search_by_projection_last_device(C.byref(cur_view), _p(Tc), C.byref(last_view), _p(Tl), fx, fy, cx, cy,
                                                    mbf, mb, th, int(mono), int(check_ori), d_kp_to_mp, d_counts,
                                                    device_id, stream))


class MapPointTable:
    """Device-resident MapPoint table keyed by mnId (orbgpu_mappoint_table_*)."""

    def __init__(self, initial_rows=0, device_id=0):
        self.L = lib()
        self.h = C.c_void_p()
        check(self.L.orbgpu_mappoint_table_create(device_id, int(initial_rows), C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.orbgpu_mappoint_table_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self):
        v = C.c_int32()
        check(self.L.orbgpu_mappoint_table_rows(self.h, C.byref(v)))
        return v.value

    def upsert(self, ids, world_pos=None, normal=None, min_dist=None, max_dist=None, desc=None, n_obs=None):
        ids = np.ascontiguousarray(ids, np.int64)
        keep = [ids]

        def arr(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            return _p(a)
        self.L.orbgpu_mappoint_table_upsert.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7
        check(self.L.orbgpu_mappoint_table_upsert(self.h, len(ids), _p(ids), arr(world_pos, np.float32), arr(normal, np.float32),
                                                  arr(min_dist, np.float32), arr(max_dist, np.float32), arr(desc, np.uint8),
                                                  arr(n_obs, np.int32)))

    def set_bad(self, ids):
        ids = np.ascontiguousarray(ids, np.int64)
        k = C.c_int32()
        self.L.orbgpu_mappoint_table_set_bad.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        check(self.L.orbgpu_mappoint_table_set_bad(self.h, len(ids), _p(ids), C.byref(k)))
        return k.value

    def set_observations(self, ids, n_obs):
        ids = np.ascontiguousarray(ids, np.int64)
        n_obs = np.ascontiguousarray(n_obs, np.int32)
        k = C.c_int32()
        self.L.orbgpu_mappoint_table_set_observations.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        check(self.L.orbgpu_mappoint_table_set_observations(self.h, len(ids), _p(ids), _p(n_obs), C.byref(k)))
        return k.value

    def retain(self, ids):
        """Keeps only the listed ids (rows renumbered densely, capacity shrunk); returns the number of rows released."""
        ids = np.ascontiguousarray(ids, np.int64)
        d = C.c_int32()
        self.L.orbgpu_mappoint_table_retain.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        check(self.L.orbgpu_mappoint_table_retain(self.h, len(ids), _p(ids), C.byref(d)))
        return d.value

    def last_unknown(self):
        """(list ids, key-point ids) of the last search call over the table that the table did not know."""
        a, b = C.c_int32(), C.c_int32()
        self.L.orbgpu_mappoint_table_last_unknown.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        check(self.L.orbgpu_mappoint_table_last_unknown(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def read(self, id_):
        wp, nr, ds = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(32, np.uint8)
        mn, mx, ob, bad = C.c_float(), C.c_float(), C.c_int32(), C.c_int32()
        self.L.orbgpu_mappoint_table_read.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7
        check(self.L.orbgpu_mappoint_table_read(self.h, int(id_), _p(wp), _p(nr), C.byref(mn), C.byref(mx), _p(ds), C.byref(ob),
                                                C.byref(bad)))
        return {"world_pos": wp, "normal": nr, "min_dist": mn.value, "max_dist": mx.value, "desc": ds,
                "has_observations": ob.value, "bad": bad.value}

    def refresh(self, graph, mp_ids, ref_kf_ids, what=REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH, outputs=(), initial=None):
        """CovisibilityGraph.refresh_points with the positions taken from the table's rows and the results written into
        them on the device; `outputs` names the optional host copies (REFRESH_OUTPUTS for all).  The caller serialises both
        handles."""
        ids = np.ascontiguousarray(mp_ids, np.int64).reshape(-1)
        return _refresh_call(self.L.orbgpu_mappoint_table_refresh, (self.h, graph.h), ids, ref_kf_ids, (), what, outputs, initial)


class DeviceFrame:
    """A Frame's matcher-side members uploaded once and kept on the device (orbgpu_frame_*)."""

    def __init__(self, device_id=0):
        self.L = lib()
        self.h = C.c_void_p()
        self.n = 0
        check(self.L.orbgpu_frame_create(device_id, C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.orbgpu_frame_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, frame):
        """frame: lib.Frame (host SoA)."""
        v = frame.view()
        self.L.orbgpu_frame_upload.argtypes = [C.c_void_p, C.c_void_p]
        check(self.L.orbgpu_frame_upload(self.h, C.byref(v)))
        self.n = frame.n
        return self

    def device_view(self):
        v, n = DeviceFrameView(), C.c_int32()
        self.L.orbgpu_frame_device_view.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        check(self.L.orbgpu_frame_device_view(self.h, C.byref(v), C.byref(n)))
        return v, n.value


def search_local_points_table(dframe, table, ids, Tcw, fx, fy, cx, cy, mbf, log_sf, th, nnratio, skip=None, scratch=None,
                              kp_ids=None, want_track=False, cos_limit=0.5):
    """Tracking::SearchLocalPoints over the MapPoint table (orbgpu_search_local_points_table).
    scratch: dict with in_view, level, view_cos, proj_x, proj_y, proj_xr (the mTrack* members filled on the host) or None
    (isInFrustum on the device).  Returns (nmatches, kp_to_mp[, track dict])."""
    L = lib()
    ids = np.ascontiguousarray(ids, np.int64)
    m, n = len(ids), dframe.n
    keep = []

    def arr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return _p(a)
    mv = None
    if scratch is not None:
        mv = MapPointView()
        mv.m = m
        mv.in_view, mv.level, mv.view_cos = arr(scratch["in_view"], np.uint8), arr(scratch["level"], np.int32), arr(scratch["view_cos"], np.float32)
        mv.proj_x, mv.proj_y, mv.proj_xr = (arr(scratch["proj_x"], np.float32), arr(scratch["proj_y"], np.float32),
                                            arr(scratch["proj_xr"], np.float32))
    T = np.ascontiguousarray(Tcw, np.float32) if Tcw is not None else None
    out = np.zeros(max(n, 1), np.int32)
    nm = C.c_int32()
    trk, ts = None, None
    if want_track:
        trk = {"in_view": np.zeros(m, np.uint8), "proj_x": np.zeros(m, np.float32), "proj_y": np.zeros(m, np.float32),
               "proj_xr": np.zeros(m, np.float32), "view_cos": np.zeros(m, np.float32), "level": np.zeros(m, np.int32)}
        ts = TrackScratch()
        for k in trk:
            setattr(ts, k, _p(trk[k]))
    L.orbgpu_search_local_points_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p] + [C.c_float] * 9 + [C.c_void_p] * 4
    check(L.orbgpu_search_local_points_table(dframe.h, table.h, m, _p(ids), arr(skip, np.uint8),
                                             C.byref(mv) if mv is not None else None, _p(T) if T is not None else None,
                                             fx, fy, cx, cy, mbf, log_sf, cos_limit, th, nnratio, arr(kp_ids, np.int64), _p(out),
                                             C.byref(nm), C.byref(ts) if ts is not None else None))
    return (nm.value, out[:n], trk) if want_track else (nm.value, out[:n])


def search_by_projection_last_table(cur, cur_Tcw, last, last_Tcw, table, last_ids, fx, fy, cx, cy, mbf, mb, th, mono,
                                    check_ori, last_outlier=None, cur_kp_ids=None):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) over the MapPoint table; cur / last: DeviceFrame."""
    L = lib()
    last_ids = np.ascontiguousarray(last_ids, np.int64)
    lo = np.ascontiguousarray(last_outlier, np.uint8) if last_outlier is not None else None
    ck = np.ascontiguousarray(cur_kp_ids, np.int64) if cur_kp_ids is not None else None
    Tc, Tl = np.ascontiguousarray(cur_Tcw, np.float32), np.ascontiguousarray(last_Tcw, np.float32)
    out = np.zeros(max(cur.n, 1), np.int32)
    nm = C.c_int32()
    L.orbgpu_search_by_projection_last_table.argtypes = [C.c_void_p] * 8 + [C.c_float] * 7 + [C.c_int32, C.c_int32, C.c_void_p,
                                                                                              C.c_void_p]
    check(L.orbgpu_search_by_projection_last_table(cur.h, _p(Tc), last.h, _p(Tl), table.h, _p(last_ids),
                                                   _p(lo) if lo is not None else None, _p(ck) if ck is not None else None,
                                                   fx, fy, cx, cy, mbf, mb, th, int(mono), int(check_ori), _p(out), C.byref(nm)))
    return nm.value, out[:cur.n]


def pose_optimization(frame, has_mp, world_pos, Tcw, inv_level_sigma2, fx, fy, cx, cy, mbf, outlier=None, device_id=0):
    """Optimizer::PoseOptimization on host arrays (orbgpu_pose_optimization).  frame: lib.Frame; has_mp [n], world_pos
    [n][3] per key point; outlier [n] uint8 or None (zeros): only edges are written.  Returns (n_inliers, Tcw 4x4 float32,
    outlier, result dict)."""
    L = lib()
    v = frame.view()
    n = frame.n
    hm = np.ascontiguousarray(has_mp, np.uint8)
    wp = np.ascontiguousarray(world_pos, np.float32).reshape(-1, 3)
    if len(hm) != n or len(wp) != n:
        raise ValueError("has_mp / world_pos must have one entry per key point")
    T = np.array(Tcw, np.float32).reshape(4, 4).copy()
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32)
    v.nlevels = len(sg)
    out = np.zeros(max(n, 1), np.uint8) if outlier is None else np.array(outlier, np.uint8)
    ni, res = C.c_int32(), PoseResult()
    L.orbgpu_pose_optimization.argtypes = [C.c_void_p] * 5 + [C.c_float] * 5 + [C.c_void_p] * 3 + [C.c_int32]
    check(L.orbgpu_pose_optimization(C.byref(v), _p(hm), _p(wp), _p(T), _p(sg), fx, fy, cx, cy, mbf, _p(out), C.byref(ni),
                                     C.byref(res), device_id))
    return ni.value, T, out[:n], res.as_dict()


def _pose_problem(p, keep):
    """A PoseProblem from a dict; keep takes the host arrays it points to."""
    q = PoseProblem()
    T = np.ascontiguousarray(p["Tcw"], np.float32)
    sg = np.ascontiguousarray(p["inv_level_sigma2"], np.float32)
    keep += [T, sg]
    q.frame = C.addressof(p["frame"])
    q.d_kp_to_mp, q.d_world_pos, q.rows = p["d_kp_to_mp"], p["d_world_pos"], int(p["rows"])
    q.Tcw, q.inv_level_sigma2 = T.ctypes.data, sg.ctypes.data
    q.fx, q.fy, q.cx, q.cy, q.mbf = p["fx"], p["fy"], p["cx"], p["cy"], p["mbf"]
    q.d_outlier, q.d_result = p["d_outlier"], p["d_result"]
    return q


def pose_optimization_batch_device(problems, stream=0, device_id=0):
    """n independent Optimizer::PoseOptimization problems in one launch (orbgpu_pose_optimization_batch_device); not
    synchronised.  problems: list of dicts with frame (DeviceFrameView), d_kp_to_mp, d_world_pos, rows, Tcw (4x4),
    inv_level_sigma2, fx, fy, cx, cy, mbf, d_outlier, d_result (device pointers; d_result holds a PoseResult)."""
    keep = []
    _batch_device("pose_optimization", PoseProblem, lambda p: _pose_problem(p, keep), problems, stream, device_id)


def pose_optimization_device(problem, stream=0, device_id=0):
    """One problem (orbgpu_pose_optimization_device); see pose_optimization_batch_device."""
    keep = []
    _one_device("pose_optimization", _pose_problem(problem, keep), stream, device_id)


def pose_optimization_table(dframe, table, kp_ids, Tcw, inv_level_sigma2, fx, fy, cx, cy, mbf, outlier=None):
    """Optimizer::PoseOptimization over the MapPoint table (orbgpu_pose_optimization_table): dframe a DeviceFrame,
    kp_ids [n] = mnId of the key point's map point or -1.  Returns (n_inliers, Tcw, outlier, result dict)."""
    L = lib()
    n = dframe.n
    ids = np.ascontiguousarray(kp_ids, np.int64)
    if len(ids) != n:
        raise ValueError("kp_ids must have one entry per key point")
    T = np.array(Tcw, np.float32).reshape(4, 4).copy()
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32)
    out = np.zeros(max(n, 1), np.uint8) if outlier is None else np.array(outlier, np.uint8)
    ni, res = C.c_int32(), PoseResult()
    L.orbgpu_pose_optimization_table.argtypes = [C.c_void_p] * 5 + [C.c_float] * 5 + [C.c_void_p] * 3
    check(L.orbgpu_pose_optimization_table(dframe.h, table.h, _p(ids), _p(T), _p(sg), fx, fy, cx, cy, mbf, _p(out),
                                           C.byref(ni), C.byref(res)))
    return ni.value, T, out[:n], res.as_dict()


def _last_spills(name, device_id):
    fn = getattr(lib(), "orbgpu_%s_last_spills" % name)
    fn.argtypes = [C.c_int32, C.c_void_p]
    v = C.c_int32()
    check(fn(device_id, C.byref(v)))
    return v.value


def pose_last_spills(device_id=0):
    """Problems of this thread's most recent pose optimisation that took the global-memory spill path."""
    return _last_spills("pose", device_id)


def _start(a, shape, t):
    """An in/out array of a host flavour: zeros, or a copy of what the caller starts from"""
    return np.zeros(shape, t) if a is None else np.array(a, t).reshape(shape).copy()


_LBA_HOST = (("Tcw", np.float32), ("fixed", np.uint8), ("cam", np.float32), ("inv_level_sigma2", np.float32),
             ("world_pos", np.float32), ("edge_point", np.int32), ("edge_pose", np.int32), ("edge_octave", np.int32),
             ("edge_xy", np.float32), ("edge_u_right", np.float32))
_LBA_PTRS = ("d_stop", "d_Tcw_d", "d_Tcw", "d_pos_d", "d_pos", "d_erase", "d_result")


def _fill_ba_problem(q, p, keep, ptrs):
    """The ten host arrays, the counts that follow them and the device pointers `ptrs` of either bundle adjustment"""
    a = {k: np.ascontiguousarray(p[k], t) for k, t in _LBA_HOST}
    keep.append(a)
    q.n_poses = int(p.get("n_poses", a["Tcw"].size // 16))
    q.n_points = int(p.get("n_points", a["world_pos"].size // 3))
    q.n_edges = int(p.get("n_edges", a["edge_point"].size))
    q.nlevels = int(p.get("nlevels", a["inv_level_sigma2"].size // max(q.n_poses, 1)))
    for k, _ in _LBA_HOST:
        setattr(q, k, a[k].ctypes.data if a[k].size else None)
    _set_pointers(q, p, ptrs)
    return q


def local_ba_problem(p, keep):
    """A LocalBAProblem from a dict: Tcw [P][4][4] (the n_local local key frames first, then the fixed cameras), fixed
    [n_local], cam [P][5] (fx, fy, cx, cy, mbf), inv_level_sigma2 [P][nlevels], world_pos [M][3], edge_point / edge_pose /
    edge_octave [E], edge_xy [E][2], edge_u_right [E] (host arrays) and the device pointers d_stop (or None), d_Tcw_d,
    d_Tcw, d_pos_d, d_pos, d_erase, d_result (holds a LocalBAResult).  The counts follow the arrays unless the dict names
    them (n_poses, n_points, n_edges, nlevels); keep takes the host arrays the structure points to."""
    q = LocalBAProblem()
    q.n_local = int(p["n_local"])
    return _fill_ba_problem(q, p, keep, _LBA_PTRS)


def local_ba_batch_device(problems, stream=0, device_id=0):
    """n independent Optimizer::LocalBundleAdjustment problems in ONE launch (orbgpu_local_ba_batch_device); enqueued, not
    synchronised.  problems: dicts as local_ba_problem takes them."""
    keep = []
    _batch_device("local_ba", LocalBAProblem, lambda p: local_ba_problem(p, keep), problems, stream, device_id)


def local_ba_device(problem, stream=0, device_id=0):
    """One problem (orbgpu_local_ba_device); see local_ba_batch_device."""
    keep = []
    _one_device("local_ba", local_ba_problem(problem, keep), stream, device_id)


def local_ba(problem, stop=None, Tcw_d=None, Tcw=None, pos_d=None, pos=None, erase=None, device_id=0):
    """Optimizer::LocalBundleAdjustment over host arrays (orbgpu_local_ba); problem: the host part of the dict
    local_ba_problem takes.  stop: None or an int sampled at the call.  The outputs start from the arrays given (zeros
    by default): a stopped call and a skipped edge leave them as they were.  Returns (Tcw_d [n_local][4][4], Tcw, pos_d
    [M][3], pos, erase [E], result dict)."""
    keep = []
    q = local_ba_problem(problem, keep)
    nl, M, E = q.n_local, q.n_points, q.n_edges
    Td, T = _start(Tcw_d, (max(nl, 1), 4, 4), np.float64), _start(Tcw, (max(nl, 1), 4, 4), np.float32)
    Xd, X = _start(pos_d, (max(M, 1), 3), np.float64), _start(pos, (max(M, 1), 3), np.float32)
    er = _start(erase, (max(E, 1),), np.uint8)
    sv = None if stop is None else C.c_int32(int(stop))
    res = LocalBAResult()
    L = lib()
    L.orbgpu_local_ba.argtypes = [C.c_void_p] * 8 + [C.c_int32]
    check(L.orbgpu_local_ba(C.byref(q), None if sv is None else C.byref(sv), _p(Td), _p(T), _p(Xd), _p(X), _p(er),
                            C.byref(res), device_id))
    return Td[:nl], T[:nl], Xd[:M], X[:M], er[:E], res.as_dict()


def local_ba_last_spills(device_id=0):
    """Problems of this thread's most recent local bundle adjustment whose reduced system lived in global memory."""
    return _last_spills("local_ba", device_id)


_BA_PTRS = ("d_stop", "d_Tcw_d", "d_Tcw", "d_pos_d", "d_pos", "d_not_included", "d_result")


def bundle_adjustment_problem(p, keep):
    """A BundleAdjustmentProblem from a dict: the host arrays of local_ba_problem with fixed [P] (one flag per pose row, no
    n_local), n_iterations (default 20) and robust (default True), and the device pointers d_stop (or None), d_Tcw_d, d_Tcw
    ([P][16]), d_pos_d, d_pos, d_not_included ([M]), d_result (holds a BundleAdjustmentResult).  The counts follow the arrays
    unless the dict names them; keep takes the host arrays the structure points to."""
    q = BundleAdjustmentProblem()
    q.n_iterations, q.robust = int(p.get("n_iterations", 20)), int(bool(p.get("robust", True)))
    return _fill_ba_problem(q, p, keep, _BA_PTRS)


def bundle_adjustment_batch_device(problems, stream=0, device_id=0):
    """n independent Optimizer::BundleAdjustment problems in ONE launch (orbgpu_bundle_adjustment_batch_device); enqueued,
    not synchronised.  problems: dicts as bundle_adjustment_problem takes them."""
    keep = []
    _batch_device("bundle_adjustment", BundleAdjustmentProblem, lambda p: bundle_adjustment_problem(p, keep), problems, stream,
                  device_id)


def bundle_adjustment_device(problem, stream=0, device_id=0):
    """One problem (orbgpu_bundle_adjustment_device); see bundle_adjustment_batch_device."""
    keep = []
    _one_device("bundle_adjustment", bundle_adjustment_problem(problem, keep), stream, device_id)


def bundle_adjustment(problem, stop=None, Tcw_d=None, Tcw=None, pos_d=None, pos=None, not_included=None, device_id=0):
    """Optimizer::BundleAdjustment over host arrays (orbgpu_bundle_adjustment); problem: the host part of the dict
    bundle_adjustment_problem takes.  stop: None or an int sampled at the call.  The outputs start from the arrays given
    (zeros by default): a call stopped at once leaves them as they were.  Returns (Tcw_d [P][4][4], Tcw, pos_d [M][3], pos,
    not_included [M], result dict)."""
    keep = []
    q = bundle_adjustment_problem(problem, keep)
    P, M = q.n_poses, q.n_points
    Td, T = _start(Tcw_d, (max(P, 1), 4, 4), np.float64), _start(Tcw, (max(P, 1), 4, 4), np.float32)
    Xd, X = _start(pos_d, (max(M, 1), 3), np.float64), _start(pos, (max(M, 1), 3), np.float32)
    ni = _start(not_included, (max(M, 1),), np.uint8)
    sv = None if stop is None else C.c_int32(int(stop))
    res = BundleAdjustmentResult()
    L = lib()
    L.orbgpu_bundle_adjustment.argtypes = [C.c_void_p] * 8 + [C.c_int32]
    check(L.orbgpu_bundle_adjustment(C.byref(q), None if sv is None else C.byref(sv), _p(Td), _p(T), _p(Xd), _p(X), _p(ni),
                                     C.byref(res), device_id))
    return Td[:P], T[:P], Xd[:M], X[:M], ni[:M], res.as_dict()


def bundle_adjustment_last_spills(device_id=0):
    """Problems of this thread's most recent bundle adjustment whose reduced system lived in global memory."""
    return _last_spills("bundle_adjustment", device_id)


_EG_HOST = (("Scw", np.float64), ("Snc", np.float64), ("fixed", np.uint8), ("edge_i", np.int32), ("edge_j", np.int32),
            ("edge_kind", np.int32))
_EG_PTRS = ("d_stop", "d_Siw_d", "d_Tiw", "d_result")


def essential_graph_problem(p, keep):
    """An EssentialGraphProblem from a dict: Scw, Snc [V][8] (qx, qy, qz, qw, tx, ty, tz, s), fixed [V], edge_i / edge_j /
    edge_kind [E] (host arrays), n_iterations (default 20), fix_scale (default False) and the device pointers d_stop (or
    None), d_Siw_d ([V][8]), d_Tiw ([V][16]), d_result (holds an EssentialGraphResult).  The counts follow the arrays
    unless the dict names them (n_vertices, n_edges); keep takes the host arrays the structure points to."""
    q = EssentialGraphProblem()
    a = {k: np.ascontiguousarray(p[k], t) for k, t in _EG_HOST}
    keep.append(a)
    q.n_vertices = int(p.get("n_vertices", a["Scw"].size // 8))
    q.n_edges = int(p.get("n_edges", a["edge_i"].size))
    q.n_iterations, q.fix_scale = int(p.get("n_iterations", 20)), int(bool(p.get("fix_scale", False)))
    for k, _ in _EG_HOST:
        setattr(q, k, a[k].ctypes.data if a[k].size else None)
    _set_pointers(q, p, _EG_PTRS)
    return q


def essential_graph_batch_device(problems, stream=0, device_id=0):
    """n independent Optimizer::OptimizeEssentialGraph problems in ONE launch (orbgpu_essential_graph_batch_device);
    enqueued, not synchronised.  problems: dicts as essential_graph_problem takes them."""
    keep = []
    _batch_device("essential_graph", EssentialGraphProblem, lambda p: essential_graph_problem(p, keep), problems, stream,
                  device_id)


def essential_graph_device(problem, stream=0, device_id=0):
    """One problem (orbgpu_essential_graph_device); see essential_graph_batch_device."""
    keep = []
    _one_device("essential_graph", essential_graph_problem(problem, keep), stream, device_id)


def essential_graph_correct_points_device(n_vertices, d_Scw, d_Siw, n_points, d_pos_in, d_ref, d_pos_out, d_n_bad_ref=None,
                                          stream=0, device_id=0):
    """G11 alone over device pointers (orbgpu_essential_graph_correct_points_device); enqueued, not synchronised."""
    L = lib()
    L.orbgpu_essential_graph_correct_points_device.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    check(L.orbgpu_essential_graph_correct_points_device(int(n_vertices), d_Scw or None, d_Siw or None, int(n_points),
                                                         d_pos_in or None, d_ref or None, d_pos_out or None,
                                                         d_n_bad_ref or None, device_id, stream))


def essential_graph(problem, stop=None, Siw_d=None, Tiw=None, world_pos=None, point_ref=None, pos_out=None, device_id=0):
    """Optimizer::OptimizeEssentialGraph over host arrays (orbgpu_essential_graph); problem: the host part of the dict
    essential_graph_problem takes.  stop: None or an int sampled at the call.  world_pos [M][3] / point_ref [M]: the map
    points to correct (G11), or None.  The outputs start from the arrays given (zeros by default; pos_out from world_pos):
    a call stopped at once leaves them as they were.  Returns (Siw_d [V][8], Tiw [V][4][4], pos [M][3], result dict)."""
    keep = []
    q = essential_graph_problem(problem, keep)
    V = q.n_vertices
    X = np.zeros((0, 3), np.float32) if world_pos is None else np.ascontiguousarray(world_pos, np.float32).reshape(-1, 3)
    M = len(X)
    ref = np.ascontiguousarray(np.zeros(0) if point_ref is None else point_ref, np.int32)
    if len(ref) != M:
        raise ValueError("point_ref must have one entry per point")
    Sd, T = _start(Siw_d, (max(V, 1), 8), np.float64), _start(Tiw, (max(V, 1), 4, 4), np.float32)
    out = _start(X if pos_out is None and M else pos_out, (max(M, 1), 3), np.float32)
    sv = None if stop is None else C.c_int32(int(stop))
    res = EssentialGraphResult()
    L = lib()
    L.orbgpu_essential_graph.argtypes = [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32]
    check(L.orbgpu_essential_graph(C.byref(q), None if sv is None else C.byref(sv), _p(Sd), _p(T), M, _p(X) if M else None,
                                   _p(ref) if M else None, _p(out) if M else None, C.byref(res), device_id))
    return Sd[:V], T[:V], out[:M], res.as_dict()


def sim3_from_pose(Tcw):
    """Sim3(Rcw, tcw, 1) of a float pose as 8 doubles (orbgpu_sim3_from_pose; host only, needs no device)."""
    L = lib()
    L.orbgpu_sim3_from_pose.argtypes = [C.c_void_p, C.c_void_p]
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    out = np.zeros(8, np.float64)
    check(L.orbgpu_sim3_from_pose(_p(T), _p(out)))
    return out


def sim3_ransac_iterations(n, probability, min_inliers, max_iterations):
    """mRansacMaxIts of Sim3Solver::SetRansacParameters (orbgpu_sim3_ransac_iterations; host only, needs no device)."""
    L = lib()
    L.orbgpu_sim3_ransac_iterations.argtypes = [C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p]
    v = C.c_int32()
    check(L.orbgpu_sim3_ransac_iterations(n, probability, min_inliers, max_iterations, C.byref(v)))
    return v.value


_SIM3_PTRS = ("valid", "Xw1", "Xw2", "octave1", "octave2", "triples", "counts", "R", "t", "s", "T12", "masks", "indices1",
              "result")


def sim3_problem(p):
    """A Sim3Problem from a dict: n1, n_hyp, T1w, T2w (4x4), K1, K2 (fx, fy, cx, cy), level_sigma2, fix_scale,
    probability, min_inliers, max_iterations, optional start_iteration / best_so_far, and the array pointers of
    include/orbgpu.h as integers (device or host addresses; missing ones are NULL)."""
    q = Sim3Problem()
    q.n1, q.n_hyp = int(p["n1"]), int(p["n_hyp"])
    _set_pointers(q, p, _SIM3_PTRS)
    _set_floats(q.T1w, p["T1w"]), _set_floats(q.T2w, p["T2w"])
    _set_intrinsics(q, p["K1"], "1"), _set_intrinsics(q, p["K2"], "2")
    _set_levels(q, p, "level_sigma2")
    q.fix_scale, q.min_inliers, q.max_iterations = int(p["fix_scale"]), int(p["min_inliers"]), int(p["max_iterations"])
    q.probability = float(p["probability"])
    q.start_iteration, q.best_so_far = int(p.get("start_iteration", 0)), int(p.get("best_so_far", 0))
    return q


def sim3_solve_batch_device(problems, stream=0, device_id=0):
    """All candidates of a LoopClosing::ComputeSim3 call in one launch sequence (orbgpu_sim3_solve_batch_device).
    problems: dicts as sim3_problem takes them, with device pointers.  Waits once for the stream (N is read back to compute
    max_its on the host); the hypotheses and the acceptance scan are enqueued and not waited for."""
    _batch_device("sim3_solve", Sim3Problem, sim3_problem, problems, stream, device_id)


def sim3_solve_device(problem, stream=0, device_id=0):
    """One candidate (orbgpu_sim3_solve_device); see sim3_solve_batch_device."""
    _one_device("sim3_solve", sim3_problem(problem), stream, device_id)


def sim3_solve(valid, Xw1, Xw2, octave1, octave2, T1w, T2w, K1, K2, level_sigma2, triples, fix_scale=False,
               probability=0.99, min_inliers=6, max_iterations=300, start_iteration=0, best_so_far=0, device_id=0):
    """Sim3Solver over host arrays (orbgpu_sim3_solve): valid [n1] is the constructor's verdict per correspondence, Xw1 /
    Xw2 [n1][3] the two map points' world positions, triples [H][3] the minimal sets (indices into the kept rows).
    Returns a dict: the result record's fields, counts [H], R (3x3), t, s, T12 (4x4) of the best iteration and inliers
    [n1] of the accepted one."""
    v = np.ascontiguousarray(valid, np.uint8)
    n1 = len(v)
    x1 = np.ascontiguousarray(Xw1, np.float32).reshape(-1, 3)
    x2 = np.ascontiguousarray(Xw2, np.float32).reshape(-1, 3)
    o1, o2 = np.ascontiguousarray(octave1, np.int32), np.ascontiguousarray(octave2, np.int32)
    if not (len(x1) == len(x2) == len(o1) == len(o2) == n1):
        raise ValueError("one entry per correspondence expected")
    tr = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
    H = len(tr)
    q = sim3_problem({"n1": n1, "n_hyp": H, "valid": v.ctypes.data, "Xw1": x1.ctypes.data, "Xw2": x2.ctypes.data,
                      "octave1": o1.ctypes.data, "octave2": o2.ctypes.data, "triples": tr.ctypes.data, "T1w": T1w, "T2w": T2w,
                      "K1": K1, "K2": K2, "level_sigma2": level_sigma2, "fix_scale": fix_scale, "probability": probability,
                      "min_inliers": min_inliers, "max_iterations": max_iterations, "start_iteration": start_iteration,
                      "best_so_far": best_so_far})
    counts = np.zeros(max(H, 1), np.int32)
    R, t, s, T12 = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros(1, np.float32), np.zeros((4, 4), np.float32)
    inl, res = np.zeros(max(n1, 1), np.uint8), Sim3Result()
    L = lib()
    L.orbgpu_sim3_solve.argtypes = [C.c_void_p] * 8 + [C.c_int32]
    check(L.orbgpu_sim3_solve(C.byref(q), _p(counts), _p(R), _p(t), _p(s), _p(T12), _p(inl), C.byref(res), device_id))
    out = res.as_dict()
    out.update(counts=counts[:H], R=R, t=t, s=float(s[0]), T12=T12, inliers=inl[:n1])
    return out


def sim3_solve_all(problem_host, device_id=0):
    """Every hypothesis of one candidate over host arrays (orbgpu_sim3_solve_all).  problem_host: a dict as sim3_problem
    takes it, with HOST addresses.  Returns a dict: the result record's fields, counts [H], R [H][3][3], t [H][3], s [H],
    T12 [H][4][4], masks [H][words] uint64."""
    q = sim3_problem(problem_host)
    H, words = q.n_hyp, (q.n1 + 63) // 64
    counts = np.zeros(max(H, 1), np.int32)
    R, t, s = np.zeros((max(H, 1), 3, 3), np.float32), np.zeros((max(H, 1), 3), np.float32), np.zeros(max(H, 1), np.float32)
    T12, masks, res = np.zeros((max(H, 1), 4, 4), np.float32), np.zeros((max(H, 1), max(words, 1)), np.uint64), Sim3Result()
    L = lib()
    L.orbgpu_sim3_solve_all.argtypes = [C.c_void_p] * 8 + [C.c_int32]
    check(L.orbgpu_sim3_solve_all(C.byref(q), _p(counts), _p(R), _p(t), _p(s), _p(T12), _p(masks), C.byref(res), device_id))
    out = res.as_dict()
    out.update(counts=counts[:H], R=R[:H], t=t[:H], s=s[:H], T12=T12[:H], masks=masks[:H, :words])
    return out


_SIM3OPT_PTRS = ("valid", "Xw1", "Xw2", "octave1", "octave2", "kp1_xy", "kp2_xy", "inlier", "result")


def sim3_opt_problem(p):
    """A Sim3OptProblem from a dict: n1, T1w, T2w (4x4), K1, K2 (fx, fy, cx, cy), inv_level_sigma2, R12 (3x3), t12, s12,
    th2, fix_scale, optional nlevels, and the array pointers of include/orbgpu.h as integers (device or host addresses;
    missing ones are NULL)."""
    q = Sim3OptProblem()
    q.n1 = int(p["n1"])
    _set_pointers(q, p, _SIM3OPT_PTRS)
    _set_floats(q.T1w, p["T1w"]), _set_floats(q.T2w, p["T2w"])
    _set_intrinsics(q, p["K1"], "1"), _set_intrinsics(q, p["K2"], "2")
    _set_levels(q, p, "inv_level_sigma2")
    _set_floats(q.R12, p["R12"]), _set_floats(q.t12, p["t12"])
    q.s12, q.th2, q.fix_scale = float(np.float32(p["s12"])), float(np.float32(p["th2"])), int(bool(p["fix_scale"]))
    return q


def sim3_optimize_batch_device(problems, stream=0, device_id=0):
    """All candidates of a LoopClosing::ComputeSim3 call in ONE launch (orbgpu_sim3_optimize_batch_device); enqueued, not
    synchronised.  problems: dicts as sim3_opt_problem takes them, with device pointers; result holds a Sim3OptResult."""
    _batch_device("sim3_optimize", Sim3OptProblem, sim3_opt_problem, problems, stream, device_id)


def sim3_optimize_device(problem, stream=0, device_id=0):
    """One candidate (orbgpu_sim3_optimize_device); see sim3_optimize_batch_device."""
    _one_device("sim3_optimize", sim3_opt_problem(problem), stream, device_id)


def sim3_optimize(valid, Xw1, Xw2, octave1, octave2, kp1_xy, kp2_xy, T1w, T2w, K1, K2, inv_level_sigma2, R12, t12, s12,
                  th2=10.0, fix_scale=False, inlier=None, nlevels=None, device_id=0):
    """Optimizer::OptimizeSim3 over host arrays (orbgpu_sim3_optimize): valid [n1] is the caller's verdict per row of
    vpMatches1, Xw1 / Xw2 [n1][3] the two map points' world positions, kp1_xy / kp2_xy [n1][2] their key points
    (mvKeysUn1[i].pt, mvKeysUn2[i2].pt), (R12, t12, s12) the Sim3 to refine.  inlier [n1] is in/out (rows that are no
    correspondence keep what they held; zeros if not given).  Returns (n_inliers, inlier, result dict): the dict holds the
    refined Sim3 (R12_d / t12_d / s12_d and their float casts), T12, Scw and the counts."""
    v = np.ascontiguousarray(valid, np.uint8)
    n1 = len(v)
    x1 = np.ascontiguousarray(Xw1, np.float32).reshape(-1, 3)
    x2 = np.ascontiguousarray(Xw2, np.float32).reshape(-1, 3)
    o1, o2 = np.ascontiguousarray(octave1, np.int32), np.ascontiguousarray(octave2, np.int32)
    k1 = np.ascontiguousarray(kp1_xy, np.float32).reshape(-1, 2)
    k2 = np.ascontiguousarray(kp2_xy, np.float32).reshape(-1, 2)
    if not (len(x1) == len(x2) == len(o1) == len(o2) == len(k1) == len(k2) == n1):
        raise ValueError("one entry per row of vpMatches1 expected")
    out = np.zeros(max(n1, 1), np.uint8)
    if inlier is not None:
        out[:n1] = np.asarray(inlier, np.uint8)
    d = {"n1": n1, "valid": v.ctypes.data, "Xw1": x1.ctypes.data, "Xw2": x2.ctypes.data, "octave1": o1.ctypes.data,
         "octave2": o2.ctypes.data, "kp1_xy": k1.ctypes.data, "kp2_xy": k2.ctypes.data, "T1w": T1w, "T2w": T2w, "K1": K1,
         "K2": K2, "inv_level_sigma2": inv_level_sigma2, "R12": R12, "t12": t12, "s12": s12, "th2": th2,
         "fix_scale": fix_scale}
    if nlevels is not None:
        d["nlevels"] = nlevels
    q = sim3_opt_problem(d)
    ni, res = C.c_int32(), Sim3OptResult()
    L = lib()
    L.orbgpu_sim3_optimize.argtypes = [C.c_void_p] * 4 + [C.c_int32]
    check(L.orbgpu_sim3_optimize(C.byref(q), _p(out), C.byref(ni), C.byref(res), device_id))
    return ni.value, out[:n1], res.as_dict()


def sim3_opt_last_spills(device_id=0):
    """Problems of this thread's most recent Sim3 optimisation that took the global-memory spill path."""
    return _last_spills("sim3_opt", device_id)


def pnp_ransac_parameters(n, probability, min_inliers, max_iterations, min_set, epsilon):
    """(mRansacMinInliers, mRansacMaxIts) of PnPsolver::SetRansacParameters (orbgpu_pnp_ransac_parameters; host only)."""
    L = lib()
    L.orbgpu_pnp_ransac_parameters.argtypes = [C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                               C.c_void_p]
    a, b = C.c_int32(), C.c_int32()
    check(L.orbgpu_pnp_ransac_parameters(n, probability, min_inliers, max_iterations, min_set, epsilon, C.byref(a), C.byref(b)))
    return a.value, b.value


_PNP_PTRS = ("valid", "Xw", "kp", "octave", "sets", "counts", "Tcw", "masks", "refined_mask", "indices", "result")


def pnp_problem(p):
    """A PnpProblem from a dict: n1, n_hyp, K (fx, fy, cx, cy), level_sigma2, min_set, min_inliers, max_iterations,
    epsilon, th2, probability, optional nlevels / start_iteration / best_so_far / n_iterations, and the array pointers
    of include/orbgpu.h as integers (device or host addresses; missing ones are NULL)."""
    q = PnpProblem()
    q.n1, q.n_hyp = int(p["n1"]), int(p["n_hyp"])
    _set_pointers(q, p, _PNP_PTRS)
    _set_intrinsics(q, p["K"])
    _set_levels(q, p, "level_sigma2")
    q.min_set, q.min_inliers, q.max_iterations = int(p["min_set"]), int(p["min_inliers"]), int(p["max_iterations"])
    q.epsilon, q.th2, q.probability = float(p["epsilon"]), float(p["th2"]), float(p["probability"])
    q.start_iteration, q.best_so_far = int(p.get("start_iteration", 0)), int(p.get("best_so_far", 0))
    q.n_iterations = int(p.get("n_iterations", 0))
    return q


def pnp_solve_batch_device(problems, stream=0, device_id=0):
    """All candidates of a Tracking::Relocalization call in one launch sequence (orbgpu_pnp_solve_batch_device).
    problems: dicts as pnp_problem takes them, with device pointers.  Waits once for the stream (N is read back for the
    RANSAC parameters); the hypotheses and the acceptance scan are enqueued and not waited for."""
    _batch_device("pnp_solve", PnpProblem, pnp_problem, problems, stream, device_id)


def pnp_solve_device(problem, stream=0, device_id=0):
    """One candidate (orbgpu_pnp_solve_device); see pnp_solve_batch_device."""
    _one_device("pnp_solve", pnp_problem(problem), stream, device_id)


def _pnp_host_problem(sc, keep, **over):
    """PnpProblem over the host arrays of a scene dict (valid, Xw, kp, octave, sets, K, level_sigma2, min_set, ...)"""
    v = np.ascontiguousarray(sc["valid"], np.uint8)
    n1 = len(v)
    x = np.ascontiguousarray(sc["Xw"], np.float32).reshape(-1, 3)
    kp = np.ascontiguousarray(sc["kp"], np.float32).reshape(-1, 2)
    o = np.ascontiguousarray(sc["octave"], np.int32)
    if not (len(x) == len(kp) == len(o) == n1):
        raise ValueError("one entry per key point expected")
    st = np.ascontiguousarray(sc["sets"], np.int32).reshape(-1, int(sc["min_set"]))
    keep += [v, x, kp, o, st]
    p = {k: sc[k] for k in ("K", "level_sigma2", "min_set", "min_inliers", "max_iterations", "epsilon", "th2", "probability")}
    for k in ("nlevels", "start_iteration", "best_so_far", "n_iterations"):
        if k in sc:
            p[k] = sc[k]
    p.update(n1=n1, n_hyp=len(st), valid=v.ctypes.data, Xw=x.ctypes.data, kp=kp.ctypes.data, octave=o.ctypes.data,
             sets=st.ctypes.data)
    p.update(over)
    return pnp_problem(p)


def pnp_solve(sc, device_id=0, **over):
    """PnPsolver over host arrays (orbgpu_pnp_solve).  sc: a dict with valid [n1], Xw [n1][3], kp [n1][2], octave [n1],
    sets [H][min_set], K, level_sigma2, min_set, min_inliers, max_iterations, epsilon, th2, probability (and optionally
    start_iteration, best_so_far, n_iterations).  Returns a dict: the result record's fields, counts [H], inliers [n1]."""
    keep = []
    q = _pnp_host_problem(sc, keep, **over)
    H, n1 = q.n_hyp, q.n1
    counts, T = np.zeros(max(H, 1), np.int32), np.zeros((4, 4), np.float32)
    inl, res = np.zeros(max(n1, 1), np.uint8), PnpResult()
    L = lib()
    L.orbgpu_pnp_solve.argtypes = [C.c_void_p] * 5 + [C.c_int32]
    check(L.orbgpu_pnp_solve(C.byref(q), _p(counts), _p(T), _p(inl), C.byref(res), device_id))
    out = res.as_dict()
    out.update(counts=counts[:H], inliers=inl[:n1], Tcw_out=T)
    return out


def pnp_solve_all(sc, device_id=0, **over):
    """Every hypothesis of one candidate over host arrays (orbgpu_pnp_solve_all); sc as pnp_solve takes it.  Returns a
    dict: the result record's fields, counts [H], Tcw_all [H][4][4], masks [H][words], refined_mask [words]."""
    keep = []
    q = _pnp_host_problem(sc, keep, **over)
    H, words = q.n_hyp, (q.n1 + 63) // 64
    counts, T = np.zeros(max(H, 1), np.int32), np.zeros((max(H, 1), 4, 4), np.float32)
    masks, rm, res = np.zeros((max(H, 1), max(words, 1)), np.uint64), np.zeros(max(words, 1), np.uint64), PnpResult()
    L = lib()
    L.orbgpu_pnp_solve_all.argtypes = [C.c_void_p] * 6 + [C.c_int32]
    check(L.orbgpu_pnp_solve_all(C.byref(q), _p(counts), _p(T), _p(masks), _p(rm), C.byref(res), device_id))
    out = res.as_dict()
    out.update(counts=counts[:H], Tcw_all=T[:H], masks=masks[:H, :words], refined_mask=rm[:words])
    return out


def pnp_solve_table(dframe, table, kp_ids, sc):
    """PnPsolver over the MapPoint table (orbgpu_pnp_solve_table): dframe a DeviceFrame, kp_ids [n] = mnId of the key
    point's map point or -1, sc a dict with sets [H][min_set], K, level_sigma2 and the RANSAC parameters as pnp_solve
    takes them.  Returns a dict: the result record's fields, counts [H], inliers [n]."""
    n = dframe.n
    ids = np.ascontiguousarray(kp_ids, np.int64)
    if len(ids) != n:
        raise ValueError("kp_ids must have one entry per key point")
    st = np.ascontiguousarray(sc["sets"], np.int32).reshape(-1, int(sc["min_set"]))
    p = {k: sc[k] for k in ("K", "level_sigma2", "min_set", "min_inliers", "max_iterations", "epsilon", "th2", "probability")}
    for k in ("nlevels", "start_iteration", "best_so_far", "n_iterations"):
        if k in sc:
            p[k] = sc[k]
    p.update(n1=0, n_hyp=len(st), sets=st.ctypes.data)
    q = pnp_problem(p)
    H = len(st)
    counts, T = np.zeros(max(H, 1), np.int32), np.zeros((4, 4), np.float32)
    inl, res = np.zeros(max(n, 1), np.uint8), PnpResult()
    L = lib()
    L.orbgpu_pnp_solve_table.argtypes = [C.c_void_p] * 8
    check(L.orbgpu_pnp_solve_table(dframe.h, table.h, _p(ids), C.byref(q), _p(counts), _p(T), _p(inl), C.byref(res)))
    out = res.as_dict()
    out.update(counts=counts[:H], inliers=inl[:n], Tcw_out=T)
    return out


_INIT_PTRS = ("kp1", "kp2", "matches12", "sets", "scores_h", "scores_f", "masks_h", "masks_f", "R21", "t21", "P3D",
              "triangulated", "result")


def initializer_cos_limits(min_parallax):
    """I10: the largest cosines for which the reference's parallax is > (ReconstructF) and >= (ReconstructH)
    min_parallax (orbgpu_initializer_cos_limits; host only).  NaN where none is."""
    L = lib()
    L.orbgpu_initializer_cos_limits.argtypes = [C.c_float, C.c_void_p, C.c_void_p]
    a, b = C.c_float(), C.c_float()
    check(L.orbgpu_initializer_cos_limits(min_parallax, C.byref(a), C.byref(b)))
    return np.float32(a.value), np.float32(b.value)


def init_problem(p):
    """An InitProblem from a dict: n1, n2, n_hyp, K (fx, fy, cx, cy), optional sigma (1.0), min_parallax (1.0),
    min_triangulated (50), and the array pointers of include/orbgpu.h as integers (missing ones are NULL)."""
    q = InitProblem()
    q.n1, q.n2, q.n_hyp = int(p["n1"]), int(p["n2"]), int(p["n_hyp"])
    _set_pointers(q, p, _INIT_PTRS)
    _set_intrinsics(q, p["K"])
    q.sigma, q.min_parallax = float(p.get("sigma", 1.0)), float(p.get("min_parallax", 1.0))
    q.min_triangulated = int(p.get("min_triangulated", 50))
    return q


def initializer_batch_device(problems, stream=0, device_id=0):
    """Independent Initializer::Initialize problems in one launch sequence (orbgpu_initializer_batch_device).  problems:
    dicts as init_problem takes them, with device pointers.  Enqueued, not waited for."""
    _batch_device("initializer", InitProblem, init_problem, problems, stream, device_id)


def initializer_device(problem, stream=0, device_id=0):
    """One problem (orbgpu_initializer_device); see initializer_batch_device."""
    _one_device("initializer", init_problem(problem), stream, device_id)


def _init_host_problem(sc, keep, **over):
    """InitProblem over the host arrays of a scene dict (kp1 [n1][2], kp2 [n2][2], matches12 [n1], sets [H][8], K, ...)"""
    k1 = np.ascontiguousarray(sc["kp1"], np.float32).reshape(-1, 2)
    k2 = np.ascontiguousarray(sc["kp2"], np.float32).reshape(-1, 2)
    m = np.ascontiguousarray(sc["matches12"], np.int32)
    if len(m) != len(k1):
        raise ValueError("one match entry per key point of frame 1 expected")
    st = np.ascontiguousarray(sc["sets"], np.int32).reshape(-1, 8)
    keep += [k1, k2, m, st]
    p = {k: sc[k] for k in ("K", "sigma", "min_parallax", "min_triangulated") if k in sc}
    p.update(n1=len(k1), n2=len(k2), n_hyp=len(st), kp1=k1.ctypes.data, kp2=k2.ctypes.data, matches12=m.ctypes.data,
             sets=st.ctypes.data)
    p.update(over)
    return init_problem(p)


def initializer(sc, device_id=0, **over):
    """Initializer::Initialize over host arrays (orbgpu_initializer).  Returns a dict: the result record's fields,
    P3D [n1][3], triangulated [n1]."""
    keep = []
    q = _init_host_problem(sc, keep, **over)
    n1 = q.n1
    P, tri, res = np.zeros((max(n1, 1), 3), np.float32), np.zeros(max(n1, 1), np.uint8), InitResult()
    L = lib()
    L.orbgpu_initializer.argtypes = [C.c_void_p] * 4 + [C.c_int32]
    check(L.orbgpu_initializer(C.byref(q), _p(P), _p(tri), C.byref(res), device_id))
    out = res.as_dict()
    out.update(P3D=P[:n1], triangulated=tri[:n1])
    return out


def initializer_all(sc, device_id=0, **over):
    """As initializer, with every hypothesis (orbgpu_initializer_all): scores_h, scores_f [H], masks_h, masks_f [H][words]."""
    keep = []
    q = _init_host_problem(sc, keep, **over)
    n1, H, words = q.n1, q.n_hyp, (q.n1 + 63) // 64
    P, tri, res = np.zeros((max(n1, 1), 3), np.float32), np.zeros(max(n1, 1), np.uint8), InitResult()
    sh, sf = np.zeros(max(H, 1), np.float32), np.zeros(max(H, 1), np.float32)
    mh, mf = (np.zeros((max(H, 1), max(words, 1)), np.uint64) for _ in range(2))
    L = lib()
    L.orbgpu_initializer_all.argtypes = [C.c_void_p] * 8 + [C.c_int32]
    check(L.orbgpu_initializer_all(C.byref(q), _p(sh), _p(sf), _p(mh), _p(mf), _p(P), _p(tri), C.byref(res), device_id))
    out = res.as_dict()
    out.update(P3D=P[:n1], triangulated=tri[:n1], scores_h=sh[:H], scores_f=sf[:H], masks_h=mh[:H, :words], masks_f=mf[:H, :words])
    return out


def distinctive_descriptors(groups, device_id=0):
    """MapPoint::ComputeDistinctiveDescriptors for a list of (n_i, 32) descriptor arrays -> best index per group."""
    off = np.zeros(len(groups) + 1, np.int32)
    for i, g in enumerate(groups):
        off[i + 1] = off[i] + len(g)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint8).reshape(-1, 32) for g in groups])
                                if len(groups) else np.zeros((0, 32), np.uint8))
    out = np.zeros(max(1, len(groups)), np.int32)
    check(lib().orbgpu_distinctive_descriptors(len(groups), _p(off), _p(flat) if len(flat) else None, _p(out), device_id))
    return out[:len(groups)]


def projection_last_sweeps():
    """(claim sweeps, re-walked rows) of this thread's most recent projection match."""
    a, b = C.c_int32(), C.c_int32()
    check(lib().orbgpu_projection_last_sweeps(C.byref(a), C.byref(b)))
    return a.value, b.value


class Frame:
    """SoA view of the Frame members the matcher reads (reference include/Frame.h:100-190)."""

    def __init__(self, kp_x, kp_y, octave, angle, u_right, desc, width, height, scale_factors):
        f32 = np.float32
        self.kp_x = np.ascontiguousarray(kp_x, f32)
        self.kp_y = np.ascontiguousarray(kp_y, f32)
        self.octave = np.ascontiguousarray(octave, np.int32)
        self.angle = np.ascontiguousarray(angle, f32)
        self.u_right = np.ascontiguousarray(u_right, f32)
        self.desc = np.ascontiguousarray(desc, np.uint8)
        self.n = len(self.kp_x)
        self.min_x, self.max_x, self.min_y, self.max_y = f32(0), f32(width), f32(0), f32(height)
        self.inv_w = f32(f32(GRID_COLS) / f32(self.max_x - self.min_x))  # Frame.cc:155
        self.inv_h = f32(f32(GRID_ROWS) / f32(self.max_y - self.min_y))  # Frame.cc:156
        self.scale_factors = np.ascontiguousarray(scale_factors, f32)
        self.cell_start, self.cell_items = assign_features_to_grid(self.kp_x, self.kp_y, self.min_x, self.min_y,
                                                                   self.inv_w, self.inv_h)
        if len(self.cell_items) == 0:
            self.cell_items = np.zeros(1, np.int32)

    def view(self):
        v = FrameView()
        v.n = self.n
        v.kp_x, v.kp_y, v.kp_octave, v.kp_angle = _p(self.kp_x), _p(self.kp_y), _p(self.octave), _p(self.angle)
        v.u_right, v.desc = _p(self.u_right), _p(self.desc)
        v.min_x, v.max_x, v.min_y, v.max_y = self.min_x, self.max_x, self.min_y, self.max_y
        v.grid_inv_w, v.grid_inv_h = self.inv_w, self.inv_h
        v.scale_factors, v.nlevels = _p(self.scale_factors), len(self.scale_factors)
        v.cell_start, v.cell_items = _p(self.cell_start), _p(self.cell_items)
        return v


class ORBmatcher:
    """Mirror of ORB_SLAM2::ORBmatcher(nnratio, checkOri) (ORBmatcher.h:41-106)."""

    TH_HIGH, TH_LOW, HISTO_LENGTH = TH_HIGH, TH_LOW, HISTO_LENGTH

    def __init__(self, nnratio=0.6, checkOri=True, device_id=0):
        self.L = lib()
        self.nnratio, self.check_ori, self.device_id = float(nnratio), bool(checkOri), device_id

    @staticmethod
    def DescriptorDistance(a, b, device_id=0):
        """ORBmatcher::DescriptorDistance (ORBmatcher.h:44); a, b: [n,32] or [32] uint8."""
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
        out = np.zeros(len(a), np.int32)
        check(lib().orbgpu_hamming256(_p(a), _p(b), len(a), _p(out), device_id))
        return out

    def MatchBruteForce(self, desc_a, angle_a, desc_b, angle_b, valid_a=None, th_low=TH_LOW):
        """SearchByBoW(KF,F) with one vocabulary node (ORBmatcher.cc:159-288)."""
        desc_a = np.ascontiguousarray(desc_a, np.uint8).reshape(-1, 32)
        desc_b = np.ascontiguousarray(desc_b, np.uint8).reshape(-1, 32)
        angle_a = np.ascontiguousarray(angle_a, np.float32)
        angle_b = np.ascontiguousarray(angle_b, np.float32)
        va = None if valid_a is None else np.ascontiguousarray(valid_a, np.uint8)
        out = np.zeros(max(1, len(desc_b)), np.int32)
        n = C.c_int32()
        check(self.L.orbgpu_match_bf(_p(desc_a), _p(angle_a), _p(va), len(desc_a), _p(desc_b), _p(angle_b), len(desc_b),
                                     th_low, self.nnratio, int(self.check_ori), _p(out), C.byref(n), self.device_id))
        return n.value, out[:len(desc_b)].copy()

    def SearchByProjection(self, frame, mp, th, kp_to_mp):
        """SearchByProjection(Frame&, vector<MapPoint*>&, th) (ORBmatcher.cc:45-129).
        mp: dict of arrays in_view,bad,obs_pos,level,view_cos,proj_x,proj_y,proj_xr,desc."""
        keep = {k: np.ascontiguousarray(mp[k], dt) for k, dt in
                (("in_view", np.uint8), ("bad", np.uint8), ("obs_pos", np.uint8), ("level", np.int32),
                 ("view_cos", np.float32), ("proj_x", np.float32), ("proj_y", np.float32),
                 ("proj_xr", np.float32), ("desc", np.uint8))}
        v = MapPointView()
        v.m = len(keep["level"])
        for k in keep:
            setattr(v, k, _p(keep[k]))
        fv = frame.view()
        out = np.ascontiguousarray(kp_to_mp, np.int32).copy()
        n = C.c_int32()
        check(self.L.orbgpu_search_by_projection(C.byref(fv), C.byref(v), th, self.nnratio, _p(out), C.byref(n),
                                                 self.device_id))
        return n.value, out

    def SearchByProjectionLast(self, cur, cur_Tcw, fx, fy, cx, cy, mbf, mb, last, th, mono, kp_to_mp):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1328-1470)."""
        keep = {k: np.ascontiguousarray(last[k], dt) for k, dt in
                (("has_mp", np.uint8), ("outlier", np.uint8), ("obs_pos", np.uint8), ("world_pos", np.float32),
                 ("desc", np.uint8), ("kp_octave", np.int32), ("kp_angle", np.float32), ("Tcw", np.float32))}
        v = LastFrameView()
        v.n = len(keep["kp_octave"])
        for k in keep:
            setattr(v, k, _p(keep[k]))
        fv = cur.view()
        T = np.ascontiguousarray(cur_Tcw, np.float32)
        out = np.ascontiguousarray(kp_to_mp, np.int32).copy()
        n = C.c_int32()
        check(self.L.orbgpu_search_by_projection_last(C.byref(fv), _p(T), fx, fy, cx, cy, mbf, mb, C.byref(v), th,
                                                      int(mono), int(self.check_ori), _p(out), C.byref(n),
                                                      self.device_id))
        return n.value, out


    def SearchByProjectionKeyFrame(self, cur, cur_Tcw, fx, fy, cx, cy, log_sf, kf, th, orb_dist, kp_to_mp):
        """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1472-1599).
        kf: dict of arrays has_mp,bad,already_found,world_pos,min_dist_inv,max_dist_inv,max_dist,desc,kp_angle."""
        keep = {k: np.ascontiguousarray(kf[k], dt) for k, dt in
                (("has_mp", np.uint8), ("bad", np.uint8), ("already_found", np.uint8), ("world_pos", np.float32),
                 ("min_dist_inv", np.float32), ("max_dist_inv", np.float32), ("max_dist", np.float32),
                 ("desc", np.uint8), ("kp_angle", np.float32))}
        v = KeyFrameView()
        v.n = len(keep["has_mp"])
        for k in keep:
            setattr(v, k, _p(keep[k]))
        fv = cur.view()
        T = np.ascontiguousarray(cur_Tcw, np.float32)
        out = np.ascontiguousarray(kp_to_mp, np.int32).copy()
        n = C.c_int32()
        check(self.L.orbgpu_search_by_projection_keyframe(C.byref(fv), _p(T), fx, fy, cx, cy, log_sf, C.byref(v), th,
                                                          int(orb_dist), int(self.check_ori), _p(out), C.byref(n),
                                                          self.device_id))
        return n.value, out


def search_by_projection_sim3(kf_frame, Scw, fx, fy, cx, cy, log_sf, pts, th, kp_to_mp, device_id=0):
    """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:290-403).
    pts: dict of arrays bad, world_pos, normal, min_dist, max_dist, desc."""
    keep = {k: np.ascontiguousarray(pts[k], dt) for k, dt in
            (("bad", np.uint8), ("world_pos", np.float32), ("normal", np.float32), ("min_dist", np.float32),
             ("max_dist", np.float32), ("desc", np.uint8))}
    v = PointsView()
    v.m = len(keep["bad"])
    for k in keep:
        setattr(v, k, _p(keep[k]))
    fv = kf_frame.view()
    S = np.ascontiguousarray(Scw, np.float32)
    out = np.ascontiguousarray(kp_to_mp, np.int32).copy()
    n = C.c_int32()
    check(lib().orbgpu_search_by_projection_sim3(C.byref(fv), _p(S), fx, fy, cx, cy, log_sf, C.byref(v), int(th), _p(out),
                                                 C.byref(n), device_id))
    return n.value, out


# ---- M6: background-thread matchers ---------------------------------------------------------------------------
_PTS_FIELDS = (("bad", np.uint8), ("world_pos", np.float32), ("normal", np.float32), ("min_dist", np.float32),
               ("max_dist", np.float32), ("desc", np.uint8))


def _points_view(cls, pts):
    keep = {k: np.ascontiguousarray(pts[k], dt) for k, dt in _PTS_FIELDS}
    v = cls()
    v.m = len(keep["bad"])
    for k in keep:
        setattr(v, k, _p(keep[k]))
    return v, keep


def fuse(kf_frame, Tcw, fx, fy, cx, cy, bf, log_sf, pts, th, inv_level_sigma2, device_id=0):
    """Candidate phase of ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:825-975): best_idx per point."""
    v, keep = _points_view(PointsView, pts)
    fv = kf_frame.view()
    T = np.ascontiguousarray(Tcw, np.float32)
    inv = np.ascontiguousarray(inv_level_sigma2, np.float32)
    out = np.full(max(v.m, 1), -1, np.int32)
    n = C.c_int32()
    L = lib()
    L.orbgpu_fuse.argtypes = [C.c_void_p, C.c_void_p] + [C.c_float] * 6 + [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                                                            C.c_void_p, C.c_int32]
    check(L.orbgpu_fuse(C.byref(fv), _p(T), fx, fy, cx, cy, bf, log_sf, C.byref(v), th, _p(inv), _p(out), C.byref(n),
                        device_id))
    return n.value, out[:v.m]


def fuse_sim3(kf_frame, Scw, fx, fy, cx, cy, log_sf, pts, th, device_id=0):
    """Candidate phase of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:977-1100)."""
    v, keep = _points_view(PointsView, pts)
    fv = kf_frame.view()
    S = np.ascontiguousarray(Scw, np.float32)
    out = np.full(max(v.m, 1), -1, np.int32)
    n = C.c_int32()
    L = lib()
    L.orbgpu_fuse_sim3.argtypes = [C.c_void_p, C.c_void_p] + [C.c_float] * 5 + [C.c_void_p, C.c_float, C.c_void_p,
                                                                                 C.c_void_p, C.c_int32]
    check(L.orbgpu_fuse_sim3(C.byref(fv), _p(S), fx, fy, cx, cy, log_sf, C.byref(v), th, _p(out), C.byref(n), device_id))
    return n.value, out[:v.m]


def search_by_sim3(kf1, kf2, T1w, T2w, s12, R12, t12, fx, fy, cx, cy, log_sf1, log_sf2, pts1, already1, pts2, already2,
                   th, device_id=0):
    """ORBmatcher::SearchBySim3 (ORBmatcher.cc:1102-1326): match12 per key point of key frame 1."""
    v1, k1 = _points_view(PointsView, pts1)
    v2, k2 = _points_view(PointsView, pts2)
    f1, f2 = kf1.view(), kf2.view()
    A = [np.ascontiguousarray(a, np.float32) for a in (T1w, T2w, R12, t12)]
    a1 = None if already1 is None else np.ascontiguousarray(already1, np.uint8)
    a2 = None if already2 is None else np.ascontiguousarray(already2, np.uint8)
    out = np.full(max(v1.m, 1), -1, np.int32)
    n = C.c_int32()
    L = lib()
    L.orbgpu_search_by_sim3.argtypes = [C.c_void_p] * 4 + [C.c_float, C.c_void_p, C.c_void_p] + [C.c_float] * 6 + \
        [C.c_void_p] * 4 + [C.c_float, C.c_void_p, C.c_void_p, C.c_int32]
    check(L.orbgpu_search_by_sim3(C.byref(f1), C.byref(f2), _p(A[0]), _p(A[1]), s12, _p(A[2]), _p(A[3]), fx, fy, cx, cy,
                                  log_sf1, log_sf2, C.byref(v1), _p(a1), C.byref(v2), _p(a2), th, _p(out), C.byref(n),
                                  device_id))
    return n.value, out[:v1.m]


def search_for_triangulation(kf1, has_mp1, node1, kf2, has_mp2, node2, F12, ex, ey, level_sigma2_2, only_stereo,
                             check_ori, device_id=0):
    """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:657-823): match12 per key point of key frame 1."""
    f1, f2 = kf1.view(), kf2.view()
    h1, h2 = np.ascontiguousarray(has_mp1, np.uint8), np.ascontiguousarray(has_mp2, np.uint8)
    n1, n2 = np.ascontiguousarray(node1, np.int32), np.ascontiguousarray(node2, np.int32)
    F = np.ascontiguousarray(F12, np.float32)
    sg = np.ascontiguousarray(level_sigma2_2, np.float32)
    out = np.full(max(kf1.n, 1), -1, np.int32)
    n = C.c_int32()
    L = lib()
    L.orbgpu_search_for_triangulation.argtypes = [C.c_void_p] * 7 + [C.c_float, C.c_float, C.c_void_p, C.c_int32, C.c_int32,
                                                                     C.c_void_p, C.c_void_p, C.c_int32]
    check(L.orbgpu_search_for_triangulation(C.byref(f1), _p(h1), _p(n1), C.byref(f2), _p(h2), _p(n2), _p(F), ex, ey,
                                            _p(sg), int(only_stereo), int(check_ori), _p(out), C.byref(n), device_id))
    return n.value, out[:kf1.n]


_NP_ARRAYS = (("kp_x", np.float32), ("kp_y", np.float32), ("kp_octave", np.int32), ("kp_angle", np.float32),
              ("u_right", np.float32), ("desc", np.uint8), ("has_mp", np.uint8), ("node", np.int32), ("depth", np.float32),
              ("kp_raw", np.float32), ("cos_stereo", np.float32))


def new_points_frame(f, keep, device=False):
    """A NewPointsFrame from a dict: the arrays of include/orbgpu.h's orbgpu_new_points_frame (numpy arrays, or with
    device=True integer device addresses plus n), Tcw, Twc (4x4), K = (fx, fy, cx, cy), mbf, level_sigma2, scale_factors,
    and for a neighbour F12 (3x3), ex, ey.  invfx / invfy default to 1 / fx, 1 / fy in float as Frame.cc computes them.
    kp_angle and kp_raw may be missing or None."""
    q = NewPointsFrame()
    if device:
        q.n = int(f["n"])
        for k, _ in _NP_ARRAYS:
            setattr(q, k, f.get(k) or None)
    else:
        a = {k: (None if f.get(k) is None else np.ascontiguousarray(f[k], t)) for k, t in _NP_ARRAYS}
        keep.append(a)
        q.n = int(f.get("n", len(a["kp_x"])))
        for k, _ in _NP_ARRAYS:
            setattr(q, k, a[k].ctypes.data if a[k] is not None and a[k].size else None)
    _set_floats(q.Tcw, f["Tcw"])
    _set_floats(q.Twc, f["Twc"])
    _set_intrinsics(q, f["K"])
    q.invfx = float(f.get("invfx", np.float32(1.0) / np.float32(f["K"][0])))
    q.invfy = float(f.get("invfy", np.float32(1.0) / np.float32(f["K"][1])))
    q.mbf = float(f.get("mbf", 0.0))
    sg, sf = np.asarray(f["level_sigma2"], np.float32), np.asarray(f["scale_factors"], np.float32)
    q.nlevels = int(f.get("nlevels", len(sg)))
    for l in range(min(len(sg), MAX_LEVELS)):
        q.level_sigma2[l], q.scale_factors[l] = float(sg[l]), float(sf[l])
    if "F12" in f:
        _set_floats(q.F12, f["F12"])
        q.ex, q.ey = float(f["ex"]), float(f["ey"])
    return q


def new_points_problem(kf1, neighbours, ratio_factor, only_stereo, check_ori, keep, device=False, **ptrs):
    """A NewPointsProblem: kf1 and neighbours as new_points_frame takes them; ptrs: stop, match12, status, x3d, n_matches,
    n_created, n_done as integer addresses (None = NULL)."""
    q = NewPointsProblem()
    q.kf1 = new_points_frame(kf1, keep, device)
    arr = (NewPointsFrame * max(len(neighbours), 1))(*[new_points_frame(f, keep, device) for f in neighbours])
    keep.append(arr)
    q.neighbours = C.addressof(arr) if len(neighbours) else None
    q.nn = int(ptrs.pop("nn", len(neighbours)))
    q.only_stereo, q.check_orientation, q.ratio_factor = int(only_stereo), int(check_ori), float(ratio_factor)
    _set_pointers(q, ptrs, ("stop", "match12", "status", "x3d", "n_matches", "n_created", "n_done"))
    return q


def create_new_map_points_device(kf1, neighbours, ratio_factor, only_stereo=False, check_ori=True, stream=0, device_id=0, **ptrs):
    """LocalMapping::CreateNewMapPoints over device arrays (orbgpu_create_new_map_points_device); enqueued, not
    synchronised.  Frames as new_points_frame(device=True) takes them; ptrs: the device addresses of the outputs and of
    the optional stop flag."""
    keep = []
    _one_device("create_new_map_points", new_points_problem(kf1, neighbours, ratio_factor, only_stereo, check_ori, keep, True, **ptrs),
                stream, device_id)


def create_new_map_points(kf1, neighbours, ratio_factor, only_stereo=False, check_ori=True, stop=None, device_id=0):
    """LocalMapping::CreateNewMapPoints (LocalMapping.cc:207-452) over host arrays (orbgpu_create_new_map_points): the whole
    neighbour loop in one call.  stop: None or an int sampled at the call.  Returns a dict: match12, status [nn][n1], x3d
    [nn][n1][3], n_matches, n_created [nn], n_done."""
    keep = []
    nn, n1 = len(neighbours), int(kf1.get("n", len(kf1["kp_x"])))
    out = {"match12": np.full((nn, n1), -1, np.int32), "status": np.zeros((nn, n1), np.int32),
           "x3d": np.zeros((nn, n1, 3), np.float32), "n_matches": np.zeros(nn, np.int32), "n_created": np.zeros(nn, np.int32)}
    pad = {k: (v if v.size else np.zeros(4, v.dtype)) for k, v in out.items()}
    done = C.c_int32(0)
    sv = None if stop is None else C.c_int32(int(stop))
    q = new_points_problem(kf1, neighbours, ratio_factor, only_stereo, check_ori, keep, False,
                           stop=None if sv is None else C.addressof(sv), n_done=C.addressof(done),
                           **{k: v.ctypes.data for k, v in pad.items()})
    L = lib()
    L.orbgpu_create_new_map_points.argtypes = [C.c_void_p, C.c_int32]
    check(L.orbgpu_create_new_map_points(C.byref(q), device_id))
    out["n_done"] = done.value
    return out


def search_for_initialization(f1, f2, prev_matched, window_size, nnratio=0.9, check_ori=True, device_id=0):
    """ORBmatcher::SearchForInitialization (ORBmatcher.cc:405-520): (nmatches, matches12, updated prev_matched)."""
    v1, v2 = f1.view(), f2.view()
    pm = np.ascontiguousarray(prev_matched, np.float32).copy()
    out = np.full(max(f1.n, 1), -1, np.int32)
    n = C.c_int32()
    L = lib()
    L.orbgpu_search_for_initialization.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32,
                                                   C.c_void_p, C.c_void_p, C.c_int32]
    check(L.orbgpu_search_for_initialization(C.byref(v1), C.byref(v2), _p(pm), int(window_size), nnratio, int(check_ori),
                                             _p(out), C.byref(n), device_id))
    return n.value, out[:f1.n], pm


def search_by_bow_keyframes(desc1, angle1, valid1, node1, desc2, angle2, valid2, node2, nnratio=0.75, check_ori=True,
                            device_id=0):
    """ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cc:522-655): match12 per key point of pKF1."""
    d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
    a1, a2 = np.ascontiguousarray(angle1, np.float32), np.ascontiguousarray(angle2, np.float32)
    v1 = None if valid1 is None else np.ascontiguousarray(valid1, np.uint8)
    v2 = None if valid2 is None else np.ascontiguousarray(valid2, np.uint8)
    nd1, nd2 = np.ascontiguousarray(node1, np.int32), np.ascontiguousarray(node2, np.int32)
    out = np.full(max(len(d1), 1), -1, np.int32)
    n = C.c_int32()
    L = lib()
    L.orbgpu_search_by_bow_keyframes.argtypes = [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_float,
                                                                                                   C.c_int32, C.c_void_p,
                                                                                                   C.c_void_p, C.c_int32]
    check(L.orbgpu_search_by_bow_keyframes(_p(d1), _p(a1), _p(v1), _p(nd1), len(d1), _p(d2), _p(a2), _p(v2), _p(nd2),
                                           len(d2), nnratio, int(check_ori), _p(out), C.byref(n), device_id))
    return n.value, out[:len(d1)]


class BatchMatcher:
    """Device-resident batched brute-force matcher (orbgpu_match_bf_batch_device)."""

    def __init__(self, max_pairs, cap, device_id=0):
        self.L = lib()
        h = C.c_void_p()
        check(self.L.orbgpu_matcher_create(device_id, max_pairs, cap, C.byref(h)))
        self.h, self.max_pairs, self.cap = h, max_pairs, cap

    def close(self):
        if getattr(self, "h", None):
            self.L.orbgpu_matcher_destroy(self.h)
            self.h = None

    __del__ = close

    def match(self, pairs, cap, d_desc_a, d_angle_a, d_valid_a, d_na, d_desc_b, d_angle_b, d_nb, angle_stride,
              th_low, nnratio, check_ori, d_match_b, d_nmatches, stream=0):
        check(self.L.orbgpu_match_bf_batch_device(self.h, pairs, cap, d_desc_a, d_angle_a, d_valid_a, d_na, d_desc_b,
                                                  d_angle_b, d_nb, angle_stride, th_low, nnratio, int(check_ori),
                                                  d_match_b, d_nmatches, stream))

    def search_by_bow(self, pairs, cap, d_desc_a, d_angle_a, d_valid_a, d_node_a, d_na, d_desc_b, d_angle_b, d_node_b,
                      d_nb, angle_stride, th_low, nnratio, check_ori, d_match_b, d_nmatches, stream=0):
        """The node-wise matcher on the same layout (orbgpu_search_by_bow_batch_device): d_node_a / d_node_b are
        [pairs][cap] int32 node ids, < 0 = not in the feature vector."""
        check(self.L.orbgpu_search_by_bow_batch_device(self.h, pairs, cap, d_desc_a, d_angle_a, d_valid_a, d_node_a, d_na,
                                                       d_desc_b, d_angle_b, d_node_b, d_nb, angle_stride, th_low, nnratio,
                                                       int(check_ori), d_match_b, d_nmatches, stream))

    def last_sweeps(self, pairs):
        out = np.zeros(pairs, np.int32)
        check(self.L.orbgpu_matcher_last_sweeps(self.h, _p(out)))
        return out

    def last_launch(self):
        """Launch shape of the last call: dict of nsplit, stage_b, resolve_threads (orbgpu_matcher_last_launch)."""
        v = [C.c_int32() for _ in range(3)]
        check(self.L.orbgpu_matcher_last_launch(self.h, *[C.byref(x) for x in v]))
        return dict(nsplit=v[0].value, stage_b=v[1].value, resolve_threads=v[2].value)


# --------------------------------------------------------------------------------------------
# On-disk formats (Map::Save records, binary PCD)
# --------------------------------------------------------------------------------------------
def keyframe_record(kf_id, timestamp, Tcw, keys, desc, mappoint_index):
    """Bytes of Map::_WriteKeyFrame (Map.cc:133-183). keys: KEYPOINT_DTYPE array, mappoint_index: uint64 (2**64-1 = none)."""
    L = lib()
    L.orbgpu_keyframe_record_bytes.restype = C.c_size_t
    L.orbgpu_keyframe_record_bytes.argtypes = [C.c_int32]
    L.orbgpu_write_keyframe_record.argtypes = [C.c_uint64, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    idx = np.ascontiguousarray(mappoint_index, np.uint64)
    T = np.ascontiguousarray(Tcw, np.float32)
    n = len(keys)
    out = np.zeros(L.orbgpu_keyframe_record_bytes(n), np.uint8)
    w = C.c_size_t()
    check(L.orbgpu_write_keyframe_record(kf_id, timestamp, _p(T), n, _p(keys) if n else None, _p(desc) if n else None,
                                         _p(idx) if n else None, _p(out), len(out), C.byref(w)))
    return out[:w.value].tobytes()


def mappoint_record(mp_id, world_pos):
    L = lib()
    L.orbgpu_write_mappoint_record.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    p = np.ascontiguousarray(world_pos, np.float32)
    out = np.zeros(20, np.uint8)
    w = C.c_size_t()
    check(L.orbgpu_write_mappoint_record(mp_id, _p(p), _p(out), 20, C.byref(w)))
    return out[:w.value].tobytes()


def pcd_binary_header(n):
    L = lib()
    L.orbgpu_pcd_binary_header.argtypes = [C.c_int64, C.c_char_p, C.c_size_t, C.c_void_p]
    buf = C.create_string_buffer(512)
    w = C.c_size_t()
    check(L.orbgpu_pcd_binary_header(n, buf, 512, C.byref(w)))
    return buf.raw[:w.value]


# --------------------------------------------------------------------------------------------
# ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>, reference include/ORBVocabulary.h)
# --------------------------------------------------------------------------------------------
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)


class ORBVocabulary:
    """The vocabulary tree on the device.  parent / is_leaf / desc / weight: one row per node in the order
    TemplatedVocabulary::loadFromTextFile creates them (TemplatedVocabulary.h:1348-1437)."""

    def __init__(self, k, L, parent, is_leaf, desc, weight, weighting=TF_IDF, scoring=L1_NORM, device_id=0):
        self.L_ = lib()
        self.parent = np.ascontiguousarray(parent, np.int32)
        self.is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.weight = np.ascontiguousarray(weight, np.float64)
        self.k, self.L, self.device_id = k, L, device_id
        h = C.c_void_p()
        fn = self.L_.orbgpu_vocabulary_create
        fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                       C.c_int32, C.c_int32, C.c_void_p]
        check(fn(k, L, len(self.parent), _p(self.parent), _p(self.is_leaf), _p(self.desc), _p(self.weight), weighting,
                 scoring, device_id, C.byref(h)))
        self.h = h
        self.L_.orbgpu_bow_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 10
        self.L_.orbgpu_bow_transform_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.L_.orbgpu_vocabulary_destroy.argtypes = [C.c_void_p]
        self.L_.orbgpu_vocabulary_size.argtypes = [C.c_void_p, C.c_void_p]

    def close(self):
        if getattr(self, "h", None):
            self.L_.orbgpu_vocabulary_destroy(self.h)
            self.h = None

    __del__ = close

    def size(self):
        n = C.c_int32()
        check(self.L_.orbgpu_vocabulary_size(self.h, C.byref(n)))
        return n.value

    def transform(self, desc, levelsup=4):
        """Frame::ComputeBoW: dict with word_id, weight, node_id per feature, bow (ids, values) and the
        FeatureVector as (nodes, start, items)."""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        m = max(n, 1)
        wid, nid = np.zeros(m, np.int32), np.zeros(m, np.int32)
        wgt = np.zeros(m, np.float64)
        bid, bval = np.zeros(m, np.int32), np.zeros(m, np.float64)
        fvn, fvs, fvi = np.zeros(m, np.int32), np.zeros(m + 1, np.int32), np.zeros(m, np.int32)
        nb, nf = C.c_int32(), C.c_int32()
        check(self.L_.orbgpu_bow_transform(self.h, _p(desc), n, levelsup, _p(wid), _p(wgt), _p(nid), _p(bid), _p(bval),
                                           C.byref(nb), _p(fvn), _p(fvs), _p(fvi), C.byref(nf)))
        return {"word_id": wid[:n], "weight": wgt[:n], "node_id": nid[:n], "bow_ids": bid[:nb.value],
                "bow_vals": bval[:nb.value], "fv_nodes": fvn[:nf.value], "fv_start": fvs[:nf.value + 1],
                "fv_items": fvi[:fvs[nf.value]]}

    def transform_batch_device(self, d_desc, batch, cap, d_n, levelsup, d_word, d_weight, d_node, stream=0):
        check(self.L_.orbgpu_bow_transform_batch_device(self.h, d_desc, batch, cap, d_n, levelsup, d_word, d_weight,
                                                        d_node, stream))


class KeyFrameDatabase:
    """Device-resident KeyFrameDatabase keyed by KeyFrame::mnId (orbgpu_keyframe_db_*): BoW candidate search for loop
    detection and relocalisation.  BoW vectors are (ascending int32 word ids, float64 values) as ORBVocabulary.transform
    returns them.  The device is bound by the first call that needs it."""

    def __init__(self, n_words, scoring=L1_NORM, initial_rows=0, device_id=0):
        self.L = lib()
        self.h = C.c_void_p()
        check(self.L.orbgpu_keyframe_db_create(int(n_words), int(scoring), device_id, int(initial_rows), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.L.orbgpu_keyframe_db_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _vec(ids, vals):
        ids = np.ascontiguousarray(ids, np.int32)
        vals = np.ascontiguousarray(vals, np.float64)
        if ids.ndim != 1 or ids.shape != vals.shape:
            raise ValueError("a BoW vector is two 1-d arrays of one length")
        return ids, vals

    def clear(self):
        check(self.L.orbgpu_keyframe_db_clear(self.h))

    def size(self):
        v = C.c_int32()
        check(self.L.orbgpu_keyframe_db_size(self.h, C.byref(v)))
        return v.value

    def add(self, kf_id, bow_ids, bow_vals):
        ids, vals = self._vec(bow_ids, bow_vals)
        check(self.L.orbgpu_keyframe_db_add(self.h, int(kf_id), len(ids), _p(ids), _p(vals)))

    def erase(self, kf_ids):
        """returns how many of the ids were in the database"""
        kf_ids = np.ascontiguousarray(np.atleast_1d(kf_ids), np.int64)
        k = C.c_int32()
        check(self.L.orbgpu_keyframe_db_erase(self.h, len(kf_ids), _p(kf_ids), C.byref(k)))
        return k.value

    def set_covisibles(self, kf_id, neighbour_ids):
        nb = np.ascontiguousarray(neighbour_ids, np.int64).reshape(-1)
        check(self.L.orbgpu_keyframe_db_set_covisibles(self.h, int(kf_id), len(nb), _p(nb)))

    def score(self, bow_ids, bow_vals, kf_ids):
        ids, vals = self._vec(bow_ids, bow_vals)
        kf_ids = np.ascontiguousarray(kf_ids, np.int64).reshape(-1)
        out = np.zeros(len(kf_ids), np.float32)
        check(self.L.orbgpu_keyframe_db_score(self.h, len(ids), _p(ids), _p(vals), len(kf_ids), _p(kf_ids), _p(out)))
        return out

    def DetectLoopCandidates(self, bow_ids, bow_vals, connected_ids, min_score, capacity=None):
        """candidate ids in the reference's order; with a capacity: (ids written, full count)"""
        ids, vals = self._vec(bow_ids, bow_vals)
        conn = np.ascontiguousarray(connected_ids, np.int64).reshape(-1)
        cap = max(self.size(), 1) if capacity is None else int(capacity)
        out = np.zeros(max(cap, 1), np.int64)
        n = C.c_int32()
        check(self.L.orbgpu_keyframe_db_detect_loop(self.h, len(ids), _p(ids), _p(vals), len(conn), _p(conn), float(min_score),
                                                    cap, _p(out), C.byref(n)))
        got = out[:min(n.value, cap)].copy()
        return got if capacity is None else (got, n.value)

    def DetectRelocalizationCandidates(self, bow_ids, bow_vals, capacity=None):
        ids, vals = self._vec(bow_ids, bow_vals)
        cap = max(self.size(), 1) if capacity is None else int(capacity)
        out = np.zeros(max(cap, 1), np.int64)
        n = C.c_int32()
        check(self.L.orbgpu_keyframe_db_detect_reloc(self.h, len(ids), _p(ids), _p(vals), cap, _p(out), C.byref(n)))
        got = out[:min(n.value, cap)].copy()
        return got if capacity is None else (got, n.value)

    def debug_global_queries(self):
        """score launches of this handle that read the query from global memory, not from LDS"""
        n = C.c_int64()
        check(self.L.orbgpu_keyframe_db_debug_global_queries(self.h, C.byref(n)))
        return n.value

    def compact(self):
        """drops the erased rows and gives their space back (D1-D4): dict of the fields of orbgpu_compact_result"""
        return _compact_call(self.L.orbgpu_keyframe_db_compact, self.h)

    def last_query(self):
        """the sharing list of the most recent detect call (K1 order): dict of id, words, first_word, score, acc, best_id"""
        n = C.c_int32()
        check(self.L.orbgpu_keyframe_db_last_query(self.h, 0, None, None, None, None, None, None, C.byref(n)))
        m = max(n.value, 1)
        cols = dict(id=np.zeros(m, np.int64), words=np.zeros(m, np.int32), first_word=np.zeros(m, np.int32),
                    score=np.zeros(m, np.float32), acc=np.zeros(m, np.float32), best_id=np.zeros(m, np.int64))
        check(self.L.orbgpu_keyframe_db_last_query(self.h, n.value, _p(cols["id"]), _p(cols["words"]), _p(cols["first_word"]),
                                                   _p(cols["score"]), _p(cols["acc"]), _p(cols["best_id"]), C.byref(n)))
        return {k: v[:n.value] for k, v in cols.items()}


class CovisibilityGraph:
    """Device-resident observation graph keyed by KeyFrame::mnId (orbgpu_covis_*): the relation between key frames and map
    points, the local map of Tracking::UpdateLocalMap and the counter of KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling (conventions V1-V8 of
    include/orbgpu.h).  All ids are int64; the device is bound by the first call that needs it."""
    MAX_SLOTS = 65536
    MAX_COVISIBLES = 10

    def __init__(self, initial_rows=0, initial_slots=0, device_id=0):
        self.L = lib()
        self.h = C.c_void_p()
        check(self.L.orbgpu_covis_graph_create(device_id, int(initial_rows), int(initial_slots), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.L.orbgpu_covis_graph_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _ids(a):
        return np.ascontiguousarray(a, np.int64).reshape(-1)

    def clear(self):
        check(self.L.orbgpu_covis_graph_clear(self.h))

    def size(self):
        """(rows that are not bad, rows that are)"""
        a, b = C.c_int32(), C.c_int32()
        check(self.L.orbgpu_covis_graph_size(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def add_keyframe(self, kf_id, n_slots, mp_ids=None):
        if mp_ids is not None:
            mp_ids = self._ids(mp_ids)
            if len(mp_ids) != int(n_slots):
                raise ValueError("mp_ids holds one id per slot")
        check(self.L.orbgpu_covis_graph_add_keyframe(self.h, int(kf_id), int(n_slots), _p(mp_ids)))

    def set_slots(self, kf_ids, idx, mp_ids):
        """returns how many entries named a key frame of the graph"""
        kf_ids, mp_ids = self._ids(kf_ids), self._ids(mp_ids)
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
        if not len(kf_ids) == len(idx) == len(mp_ids):
            raise ValueError("set_slots takes three arrays of one length")
        k = C.c_int32()
        check(self.L.orbgpu_covis_graph_set_slots(self.h, len(kf_ids), _p(kf_ids), _p(idx), _p(mp_ids), C.byref(k)))
        return k.value

    def set_bad(self, kf_ids):
        kf_ids = self._ids(np.atleast_1d(kf_ids))
        k = C.c_int32()
        check(self.L.orbgpu_covis_graph_set_bad(self.h, len(kf_ids), _p(kf_ids), C.byref(k)))
        return k.value

    def set_parent(self, kf_id, parent_id):
        check(self.L.orbgpu_covis_graph_set_parent(self.h, int(kf_id), int(parent_id)))

    def set_covisibles(self, kf_id, ids):
        ids = self._ids(ids)
        check(self.L.orbgpu_covis_graph_set_covisibles(self.h, int(kf_id), len(ids), _p(ids)))

    def local_map(self, kp_ids, prev_kf_ids=(), kf_capacity=None, point_capacity=None):
        """UpdateLocalKeyFrames + UpdateLocalPoints: dict of kf_ids, point_ids (as long as the capacities allow) and the
        fields of orbgpu_covis_local_map_result"""
        kp, prev = self._ids(kp_ids), self._ids(prev_kf_ids)
        res = CovisLocalMapResult()
        if kf_capacity is None or point_capacity is None:  # the full lengths first
            check(self.L.orbgpu_covis_local_map(self.h, len(kp), _p(kp), len(prev), _p(prev), 0, None, 0, None, C.byref(res)))
            kf_capacity = res.n_kfs if kf_capacity is None else kf_capacity
            point_capacity = res.n_points if point_capacity is None else point_capacity
        kfs, pts = np.zeros(max(int(kf_capacity), 1), np.int64), np.zeros(max(int(point_capacity), 1), np.int64)
        check(self.L.orbgpu_covis_local_map(self.h, len(kp), _p(kp), len(prev), _p(prev), int(kf_capacity), _p(kfs),
                                            int(point_capacity), _p(pts), C.byref(res)))
        out = {name: getattr(res, name) for name, _ in CovisLocalMapResult._fields_}
        out["kf_ids"] = kfs[:min(res.n_kfs, int(kf_capacity))].copy()
        out["point_ids"] = pts[:min(res.n_points, int(point_capacity))].copy()
        return out

    def connections(self, kf_id, th=15, capacity=None, ordered_capacity=None):
        """UpdateConnections' counter: dict of ids, counts (ascending id), ordered_ids, ordered_weights and n, n_ordered"""
        cap = sum(self.size()) if capacity is None else int(capacity)
        ocap = cap if ordered_capacity is None else int(ordered_capacity)
        ids, counts = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int32)
        oids, ow = np.zeros(max(ocap, 1), np.int64), np.zeros(max(ocap, 1), np.int32)
        n, no = C.c_int32(), C.c_int32()
        check(self.L.orbgpu_covis_connections(self.h, int(kf_id), int(th), cap, _p(ids), _p(counts), C.byref(n), ocap, _p(oids),
                                              _p(ow), C.byref(no)))
        return dict(n=n.value, n_ordered=no.value, ids=ids[:min(n.value, cap)].copy(), counts=counts[:min(n.value, cap)].copy(),
                    ordered_ids=oids[:min(no.value, ocap)].copy(), ordered_weights=ow[:min(no.value, ocap)].copy())

    def debug_global_queries(self):
        """vote launches of this handle that read the query from global memory, not from LDS"""
        n = C.c_int64()
        check(self.L.orbgpu_covis_graph_debug_global_queries(self.h, C.byref(n)))
        return n.value

    def compact(self):
        """drops the bad rows no live row names as parent and gives their space back (C1-C7): dict of the fields of
        orbgpu_compact_result"""
        return _compact_call(self.L.orbgpu_covis_graph_compact, self.h)

    MAX_LEVELS = 16
    KP_STEREO = 0x40
    KP_FAR = 0x80

    def set_keypoints(self, kf_id, kp):
        """the attribute byte of every slot of a key frame (V1): octave | KP_STEREO | KP_FAR"""
        kp = np.ascontiguousarray([] if kp is None else kp, np.uint8).reshape(-1)
        check(self.L.orbgpu_covis_graph_set_keypoints(self.h, int(kf_id), len(kp), _p(kp)))

    def observations(self, mp_ids):
        """(n_obs, n_slots) per id: the weighted MapPoint::Observations() and the number of slots that hold the point"""
        ids = self._ids(mp_ids)
        n_obs, n_slots = np.zeros(max(len(ids), 1), np.int32), np.zeros(max(len(ids), 1), np.int32)
        check(self.L.orbgpu_covis_observations(self.h, len(ids), _p(ids), _p(n_obs), _p(n_slots)))
        return n_obs[:len(ids)].copy(), n_slots[:len(ids)].copy()

    def keyframe_culling(self, kf_ids, not_erase=None, th_obs=3, point_capacity=None):
        """LocalMapping::KeyFrameCulling (V8): dict of verdict, n_mps, n_redundant (per candidate), bad_point_ids (as long
        as point_capacity allows) and the fields of orbgpu_covis_culling_result.  The graph is not modified."""
        ids = self._ids(kf_ids)
        n = len(ids)
        ne = None
        if not_erase is not None:
            ne = np.ascontiguousarray(not_erase, np.uint8).reshape(-1)
            if len(ne) != n:
                raise ValueError("not_erase holds one flag per candidate")
        verdict, n_mps, n_red = np.zeros(max(n, 1), np.int8), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        res = CovisCullingResult()

        def call(cap, out):
            check(self.L.orbgpu_covis_keyframe_culling(self.h, n, _p(ids), _p(ne), int(th_obs), _p(verdict), _p(n_mps), _p(n_red),
                                                       int(cap), _p(out), C.byref(res)))
        if point_capacity is None:  # the full length first
            call(0, None)
            point_capacity = res.n_points_bad
        bad = np.zeros(max(int(point_capacity), 1), np.int64)
        call(point_capacity, bad)
        out = {name: getattr(res, name) for name, _ in CovisCullingResult._fields_}
        out.update(verdict=verdict[:n].copy(), n_mps=n_mps[:n].copy(), n_redundant=n_red[:n].copy(),
                   bad_point_ids=bad[:min(res.n_points_bad, int(point_capacity))].copy())
        return out

    def set_scale_factors(self, scale_factors):
        """KeyFrame::mvScaleFactors, one table per graph (R6)"""
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        check(self.L.orbgpu_covis_graph_set_scale_factors(self.h, len(sf), _p(sf)))

    def set_descriptors(self, kf_id, desc):
        """mDescriptors of a key frame, [n_slots][32] bytes, once behind add_keyframe (R4)"""
        d = np.ascontiguousarray(np.zeros((0, 32), np.uint8) if desc is None else desc, np.uint8).reshape(-1, 32)
        check(self.L.orbgpu_covis_graph_set_descriptors(self.h, int(kf_id), len(d), _p(d)))

    def set_centres(self, kf_ids, centres):
        """KeyFrame::GetCameraCenter() of a batch of key frames (R5); returns how many ids named a key frame of the graph"""
        kf_ids = self._ids(np.atleast_1d(kf_ids))
        c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
        if len(c) != len(kf_ids):
            raise ValueError("one centre per key frame")
        k = C.c_int32()
        check(self.L.orbgpu_covis_graph_set_centres(self.h, len(kf_ids), _p(kf_ids), _p(c), C.byref(k)))
        return k.value

    def refresh_points(self, mp_ids, ref_kf_ids, world_pos, what=REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH, outputs=REFRESH_OUTPUTS,
                       initial=None):
        """MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth for a batch of points (R1-R8): dict of the
        outputs named in `outputs` (in/out ones start from `initial[name]` where given), n_slots, status and the fields of
        orbgpu_covis_refresh_result.  The graph is not modified."""
        ids = self._ids(mp_ids)
        pos = np.ascontiguousarray(world_pos, np.float32).reshape(-1, 3)
        if len(pos) != len(ids):
            raise ValueError("one position per map point")
        return _refresh_call(self.L.orbgpu_covis_refresh_points, (self.h,), ids, ref_kf_ids, (_p(pos),), what, outputs, initial)


def search_by_bow(desc_kf, angle_kf, valid_kf, node_kf, desc_f, angle_f, node_f, th_low=TH_LOW, nnratio=0.7,
                  check_ori=True, device_id=0):
    """ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) on per-feature node ids (orbgpu_search_by_bow)."""
    desc_kf = np.ascontiguousarray(desc_kf, np.uint8).reshape(-1, 32)
    desc_f = np.ascontiguousarray(desc_f, np.uint8).reshape(-1, 32)
    akf, af = np.ascontiguousarray(angle_kf, np.float32), np.ascontiguousarray(angle_f, np.float32)
    nkf, nf_ = np.ascontiguousarray(node_kf, np.int32), np.ascontiguousarray(node_f, np.int32)
    va = None if valid_kf is None else np.ascontiguousarray(valid_kf, np.uint8)
    out = np.zeros(max(1, len(desc_f)), np.int32)
    n = C.c_int32()
    L = lib()
    L.orbgpu_search_by_bow.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_int32]
    check(L.orbgpu_search_by_bow(_p(desc_kf), _p(akf), _p(va), _p(nkf), len(desc_kf), _p(desc_f), _p(af), _p(nf_),
                                 len(desc_f), th_low, nnratio, int(check_ori), _p(out), C.byref(n), device_id))
    return n.value, out[:len(desc_f)].copy()


# --------------------------------------------------------------------------------------------
# PointCloudMapping (reference include/PointCloudMap.h:41-88)
# --------------------------------------------------------------------------------------------
class PointCloudMapping:
    """Arithmetic of ORB_SLAM2::PointCloudMapping: insertKeyFrame -> back-project, transform,
    append, voxel-filter the global map (PointCloudMap.cc:204-262). Thread/condvar protocol and
    viewer stay on the host side of the C++ shim."""

    def __init__(self, resolution, device_id=0):
        self.L = lib()
        h = C.c_void_p()
        check(self.L.orbgpu_cloud_create(float(resolution), device_id, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.orbgpu_cloud_destroy(self.h)
            self.h = None

    __del__ = close

    def insertKeyFrame(self, depth, rgb, fx, fy, cx, cy, Tcw):
        depth = np.ascontiguousarray(depth, np.float32)
        rgb = np.ascontiguousarray(rgb, np.uint8)
        T = np.ascontiguousarray(Tcw, np.float32)
        h, w = depth.shape
        check(self.L.orbgpu_cloud_insert(self.h, _p(depth), depth.strides[0] // 4, _p(rgb), rgb.strides[0], w, h, fx, fy,
                                         cx, cy, _p(T)))

    def insertKeyFrameDevice(self, d_depth, depth_stride, d_rgb, rgb_stride, w, h, fx, fy, cx, cy, Tcw):
        """Device-resident key frame (pointers into HBM, strides in floats / bytes)."""
        T = np.ascontiguousarray(Tcw, np.float32)
        check(self.L.orbgpu_cloud_insert_device(self.h, d_depth, depth_stride, d_rgb, rgb_stride, w, h, fx, fy, cx, cy,
                                                _p(T)))

    def set_profiling(self, on):
        check(self.L.orbgpu_cloud_set_profiling(self.h, int(on)))

    def last_insert_ms(self):
        v = C.c_float()
        check(self.L.orbgpu_cloud_last_insert_ms(self.h, C.byref(v)))
        return v.value

    def clear(self):
        self.L.orbgpu_cloud_clear.argtypes = [C.c_void_p]
        check(self.L.orbgpu_cloud_clear(self.h))

    def appendFiltered(self, depth, rgb, fx, fy, cx, cy, Tcw):
        """One iteration of the shutdown loop (PointCloudMap.cc:272-282)."""
        depth = np.ascontiguousarray(depth, np.float32)
        rgb = np.ascontiguousarray(rgb, np.uint8)
        T = np.ascontiguousarray(Tcw, np.float32)
        h, w = depth.shape
        self.L.orbgpu_cloud_append_filtered.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32,
                                                        C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
        check(self.L.orbgpu_cloud_append_filtered(self.h, _p(depth), depth.strides[0] // 4, _p(rgb), rgb.strides[0], w, h,
                                                  fx, fy, cx, cy, _p(T)))

    def remove_outliers(self, mean_k=50, stddev_mul=1.0):
        """sor.filter of the global map (PointCloudMap.cc:283-285); returns the number of points removed."""
        r = C.c_int64()
        check(self.L.orbgpu_cloud_remove_outliers(self.h, mean_k, float(stddev_mul), C.byref(r)))
        return r.value

    def save_pcd(self, path):
        self.L.orbgpu_cloud_save_pcd.argtypes = [C.c_void_p, C.c_char_p]
        check(self.L.orbgpu_cloud_save_pcd(self.h, path.encode()))

    def last_path(self):
        v = C.c_int32()
        check(self.L.orbgpu_cloud_last_path(self.h, C.byref(v)))
        return v.value

    def rebuild(self, depths, rgbs, fx, fy, cx, cy, Tcws):
        depths = [np.ascontiguousarray(d, np.float32) for d in depths]
        rgbs = [np.ascontiguousarray(r, np.uint8) for r in rgbs]
        Ts = [np.ascontiguousarray(t, np.float32) for t in Tcws]
        n = len(depths)
        h, w = depths[0].shape
        dp = (C.c_void_p * n)(*[d.ctypes.data for d in depths])
        rp = (C.c_void_p * n)(*[r.ctypes.data for r in rgbs])
        tp = (C.c_void_p * n)(*[t.ctypes.data for t in Ts])
        check(self.L.orbgpu_cloud_rebuild(self.h, n, dp, depths[0].strides[0] // 4, rp, rgbs[0].strides[0], w, h, fx, fy,
                                          cx, cy, tp))

    def size(self):
        n = C.c_int64()
        check(self.L.orbgpu_cloud_size(self.h, C.byref(n)))
        return n.value

    def download(self):
        n = self.size()
        out = np.zeros(max(1, n), POINT_DTYPE)
        got = C.c_int64()
        check(self.L.orbgpu_cloud_download(self.h, _p(out), max(1, n), C.byref(got)))
        return out[:got.value].copy()

    def last_overflow(self):
        o = C.c_int32()
        check(self.L.orbgpu_cloud_last_overflow(self.h, C.byref(o)))
        return bool(o.value)


def backproject(depth, rgb, fx, fy, cx, cy, Tcw=None, device_id=0):
    depth = np.ascontiguousarray(depth, np.float32)
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = depth.shape
    cap = ((h + 2) // 3) * ((w + 2) // 3)
    out = np.zeros(max(1, cap), POINT_DTYPE)
    n = C.c_int64()
    T = None if Tcw is None else np.ascontiguousarray(Tcw, np.float32)
    check(lib().orbgpu_backproject(_p(depth), depth.strides[0] // 4, _p(rgb), rgb.strides[0], w, h, fx, fy, cx, cy,
                                   _p(T), _p(out), max(1, cap), C.byref(n), device_id))
    return out[:n.value].copy()


def statistical_outlier_removal(points, mean_k=50, stddev_mul=1.0, device_id=0):
    """pcl::StatisticalOutlierRemoval::filter: (kept points, mean neighbour distance of every input point)."""
    points = np.ascontiguousarray(points, POINT_DTYPE)
    out = np.zeros(max(1, len(points)), POINT_DTYPE)
    md = np.zeros(max(1, len(points)), np.float32)
    n = C.c_int64()
    check(lib().orbgpu_statistical_outlier_removal(_p(points), len(points), mean_k, float(stddev_mul), _p(out),
                                                   max(1, len(points)), C.byref(n), _p(md), device_id))
    return out[:n.value].copy(), md[:len(points)].copy()


def voxel_filter(points, resolution, device_id=0):
    points = np.ascontiguousarray(points, POINT_DTYPE)
    out = np.zeros(max(1, len(points)), POINT_DTYPE)
    n = C.c_int64()
    ov = C.c_int32()
    check(lib().orbgpu_voxel_filter(_p(points), len(points), float(resolution), _p(out), max(1, len(points)),
                                    C.byref(n), C.byref(ov), device_id))
    return out[:n.value].copy(), bool(ov.value)
