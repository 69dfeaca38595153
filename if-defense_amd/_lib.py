"""ctypes binding of libifd.so (the C ABI in include/ifd.h).

The product path has NO fallback: if the HIP library is missing or does not load, importing
this module raises.  (The CPU oracle under oracle/ is test infrastructure and is never used here.)
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# IFD_LIB: another build of the same library (test hook: csrc/libifd_exact.so, the -DIFD_EXACT_REP build)
LIB_PATH = os.environ.get("IFD_LIB") or os.path.join(HERE, "csrc", "libifd.so")

IFD_OK = 0
IFD_ERR_TIMEOUT = -5
IFD_ERR_OVERFLOW = -6
ABI_VERSION = 5


class IfdConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("plane_resolution", C.c_int32), ("c_dim", C.c_int32),
                ("hidden_dim", C.c_int32), ("n_blocks", C.c_int32), ("unet_depth", C.c_int32),
                ("unet_start_filts", C.c_int32), ("padding", C.c_float)]


class IfdOptParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("steps", C.c_int32), ("t0", C.c_int32),
                ("loss_batch", C.c_int32), ("normalize", C.c_int32), ("lr", C.c_float),
                ("rep_weight", C.c_float), ("threshold", C.c_float), ("rep_radius", C.c_float),
                ("rep_h", C.c_float), ("rep_eps", C.c_float), ("knn_scan_every_step", C.c_int32),
                ("split", C.c_int32), ("planes_shared", C.c_int32), ("knn_reference_form", C.c_int32), ("precision", C.c_int32)]


class IfdPrepParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_sel", C.c_int32), ("n_opt", C.c_int32), ("padding_scale", C.c_float),
                ("init_sigma", C.c_float), ("seed", C.c_uint64), ("cloud_index_base", C.c_int64)]


class IfdMeshParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("resolution0", C.c_int32), ("upsampling_steps", C.c_int32),
                ("n_sample", C.c_int32), ("max_triangles", C.c_int32), ("padding", C.c_float), ("threshold", C.c_double),
                ("seed", C.c_uint64), ("cloud_index_base", C.c_int64), ("precision", C.c_int32), ("reserved", C.c_int32)]


# name -> (restype, argtypes); must list every symbol include/ifd.h declares (tests check this)
SIGNATURES = {
    "ifd_abi_version": (C.c_int, []),
    "ifd_weight_count": (C.c_size_t, []),
    "ifd_create": (C.c_void_p, [C.c_void_p, C.c_size_t, C.POINTER(IfdConfig), C.c_int]),
    "ifd_destroy": (None, [C.c_void_p]),
    "ifd_last_error": (C.c_char_p, [C.c_void_p]),
    "ifd_sor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                          C.c_void_p]),
    "ifd_prepare": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(IfdPrepParams),
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]),
    "ifd_encode_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "ifd_unet": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ifd_encode_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ifd_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                             C.c_void_p]),
    "ifd_decode_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    "ifd_repulsion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    "ifd_optimize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(IfdOptParams),
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ifd_get_counters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "ifd_optimize_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ifd_normalize_unit_sphere": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    # ONet-Opt variant
    "ifd_onet_weight_count": (C.c_size_t, []),
    "ifd_onet_create": (C.c_void_p, [C.c_void_p, C.c_size_t, C.c_int]),
    "ifd_onet_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ifd_onet_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "ifd_onet_decode_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "ifd_onet_optimize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(IfdOptParams),
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ifd_onet_mesh_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(IfdMeshParams), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "ifd_mc_table": (C.c_int, [C.c_void_p, C.c_void_p]),
    # validation seams of the mesh path
    "ifd_mesh_from_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_float, C.c_int, C.c_int, C.c_uint64,
                                     C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ifd_mise_from_field": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]),
}

# include/ifd_dup.h (the baseline defenses: SRS, DUP fill, PU-Net), versioned on its own
DUP_ABI_VERSION = 1


class IfdPunetAux(C.Structure):
    _fields_ = [("fps_idx", C.c_void_p), ("ball_idx", C.c_void_p), ("knn_idx", C.c_void_p)]


DUP_SIGNATURES = {
    "ifd_dup_abi_version": (C.c_int, []),
    "ifd_punet_weight_count": (C.c_size_t, []),
    "ifd_dup_create": (C.c_void_p, [C.c_void_p, C.c_size_t, C.c_int]),
    "ifd_srs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p,
                          C.c_void_p]),
    "ifd_dup_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int64, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "ifd_punet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_int64,
                                    C.c_void_p, C.POINTER(IfdPunetAux), C.c_void_p]),
}

# include/ifd_cls.h (the victim classifier: PointNet), versioned on its own
CLS_ABI_VERSION = 1
CLS_POINTNET, CLS_POINTNET2, CLS_DGCNN, CLS_POINTCONV = 0, 1, 2, 3
CLS_MAX_POINTS = 10000


class IfdClsAux(C.Structure):
    _fields_ = [("trans", C.c_void_p), ("trans_feat", C.c_void_p), ("global_feat", C.c_void_p), ("pred", C.c_void_p)]


CLS_SIGNATURES = {
    "ifd_cls_abi_version": (C.c_int, []),
    "ifd_cls_weight_count": (C.c_size_t, [C.c_int, C.c_int]),
    "ifd_cls_create": (C.c_void_p, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ifd_cls_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(IfdClsAux),
                                  C.c_void_p]),
}

# include/ifd_atk.h (input gradients of the PointNet victim and the FGM family), versioned on its own
ATK_ABI_VERSION = 1
ATK_LOSS_LOGITS, ATK_LOSS_CE = 0, 1
FGM_FGM, FGM_IFGM, FGM_MIFGM, FGM_PGD = 0, 1, 2, 3


class IfdAtkOut(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("loss", C.c_void_p), ("pred", C.c_void_p), ("win_feat", C.c_void_p),
                ("win_stn", C.c_void_p), ("global_feat", C.c_void_p)]


class IfdFgmParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("loss_kind", C.c_int32), ("num_iter", C.c_int32),
                ("kappa", C.c_float), ("scale", C.c_float), ("step_size", C.c_float), ("budget", C.c_float), ("mu", C.c_float)]


ATK_SIGNATURES = {
    "ifd_atk_abi_version": (C.c_int, []),
    "ifd_cls_input_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                     C.c_void_p, C.POINTER(IfdAtkOut), C.c_void_p]),
    "ifd_fgm_update": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                 C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ifd_fgm_attack": (C.c_int, [C.c_void_p, C.POINTER(IfdFgmParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
}

# include/ifd_cw.h (the CW point-perturbation attack on the PointNet victim), versioned on its own
CW_ABI_VERSION = 1


class IfdCwState(C.Structure):
    _fields_ = [("m", C.c_void_p), ("v", C.c_void_p), ("bestdist", C.c_void_p), ("bestscore", C.c_void_p), ("o_bestdist", C.c_void_p),
                ("o_bestscore", C.c_void_p), ("o_bestattack", C.c_void_p), ("weight", C.c_void_p), ("lower", C.c_void_p),
                ("upper", C.c_void_p)]


class IfdCwParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("loss_kind", C.c_int32), ("binary_step", C.c_int32), ("num_iter", C.c_int32),
                ("kappa", C.c_float), ("scale", C.c_float), ("attack_lr", C.c_float), ("init_weight", C.c_float),
                ("max_weight", C.c_float)]


CW_SIGNATURES = {
    "ifd_cw_abi_version": (C.c_int, []),
    "ifd_cw_step": (C.c_int, [C.c_void_p, C.POINTER(IfdCwState), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ifd_cw_adjust": (C.c_int, [C.c_void_p, C.POINTER(IfdCwState), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ifd_cw_perturb_attack": (C.c_int, [C.c_void_p, C.POINTER(IfdCwParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/ifd_knn.h (the kNN attack on the PointNet victim), versioned on its own
KNN_ABI_VERSION = 1
KNN_MIN_POINTS, KNN_MAX_POINTS = 6, 2048


class IfdKnnParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("loss_kind", C.c_int32), ("num_iter", C.c_int32), ("kappa", C.c_float), ("scale", C.c_float),
                ("attack_lr", C.c_float), ("chamfer_weight", C.c_float), ("knn_weight", C.c_float), ("alpha", C.c_float),
                ("budget", C.c_float)]


class IfdKnnDiag(C.Structure):
    _fields_ = [("info", C.c_void_p), ("dist_grad", C.c_void_p), ("nn_ori", C.c_void_p), ("nn5", C.c_void_p), ("mask", C.c_void_p)]


KNN_SIGNATURES = {
    "ifd_knn_abi_version": (C.c_int, []),
    "ifd_knn_step": (C.c_int, [C.c_void_p, C.POINTER(IfdKnnParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_int, C.c_float, C.c_float, C.POINTER(IfdKnnDiag), C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ifd_knn_project_clip": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ifd_knn_attack": (C.c_int, [C.c_void_p, C.POINTER(IfdKnnParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/ifd_add.h (the CW point-adding attack on the PointNet victim), versioned on its own
ADD_ABI_VERSION = 1
ADD_CHAMFER, ADD_HAUSDORFF = 0, 1
ADD_MAX_ADD, ADD_MAX_ORI = 1024, 2048


class IfdAddDiag(C.Structure):
    _fields_ = [("dist_grad", C.c_void_p), ("nn_ori", C.c_void_p), ("far", C.c_void_p)]


class IfdAddParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("loss_kind", C.c_int32), ("binary_step", C.c_int32),
                ("num_iter", C.c_int32), ("num_add", C.c_int32), ("kappa", C.c_float), ("scale", C.c_float), ("attack_lr", C.c_float),
                ("init_weight", C.c_float), ("max_weight", C.c_float)]


ADD_SIGNATURES = {
    "ifd_add_abi_version": (C.c_int, []),
    "ifd_add_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "ifd_add_critical_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "ifd_add_step": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(IfdCwState), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(IfdAddDiag), C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                               C.c_int, C.c_void_p]),
    "ifd_add_attack": (C.c_int, [C.c_void_p, C.POINTER(IfdAddParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/ifd_drop.h (the saliency Drop attack on the PointNet victim), versioned on its own
DROP_ABI_VERSION = 1
DROP_MAX_POINTS = 2048


class IfdDropOut(C.Structure):
    _fields_ = [("saliency", C.c_void_p), ("center", C.c_void_p), ("dropped", C.c_void_p)]


class IfdDropParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("num_drop", C.c_int32), ("k", C.c_int32), ("alpha", C.c_float), ("scale", C.c_float)]


DROP_SIGNATURES = {
    "ifd_drop_abi_version": (C.c_int, []),
    "ifd_drop_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                C.POINTER(IfdDropOut), C.c_void_p]),
    "ifd_drop_attack": (C.c_int, [C.c_void_p, C.POINTER(IfdDropParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/ifd_cluster.h (the CW cluster-adding attack on the PointNet victim), versioned on its own
CLUSTER_ABI_VERSION = 1
CLUSTER_DBSCAN_MAX_POINTS = 256


class IfdClusterDiag(C.Structure):
    _fields_ = [("dist_grad", C.c_void_p), ("nn_ori", C.c_void_p), ("far_i", C.c_void_p), ("far_j", C.c_void_p), ("far_val", C.c_void_p)]


class IfdClusterParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("loss_kind", C.c_int32), ("binary_step", C.c_int32), ("num_iter", C.c_int32),
                ("num_add", C.c_int32), ("cl_num_p", C.c_int32), ("kappa", C.c_float), ("scale", C.c_float), ("attack_lr", C.c_float),
                ("init_weight", C.c_float), ("max_weight", C.c_float)]


CLUSTER_SIGNATURES = {
    "ifd_cluster_abi_version": (C.c_int, []),
    "ifd_cluster_dbscan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "ifd_cluster_step": (C.c_int, [C.c_void_p, C.POINTER(IfdCwState), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(IfdClusterDiag), C.c_int, C.c_float, C.c_float, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ifd_cluster_attack": (C.c_int, [C.c_void_p, C.POINTER(IfdClusterParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/ifd_object.h (the CW object-adding attack on the PointNet victim), versioned on its own
OBJECT_ABI_VERSION = 1


class IfdObjectState(C.Structure):
    _fields_ = [("cw", IfdCwState), ("obj", C.c_void_p), ("shift", C.c_void_p), ("angle", C.c_void_p), ("shift_m", C.c_void_p),
                ("shift_v", C.c_void_p), ("angle_m", C.c_void_p), ("angle_v", C.c_void_p)]


class IfdObjectDiag(C.Structure):
    _fields_ = [("obj_grad", C.c_void_p), ("nn_ori", C.c_void_p), ("g_shift", C.c_void_p), ("g_angle", C.c_void_p), ("l2", C.c_void_p),
                ("cd", C.c_void_p)]


class IfdObjectParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("loss_kind", C.c_int32), ("binary_step", C.c_int32), ("num_iter", C.c_int32),
                ("num_add", C.c_int32), ("obj_num_p", C.c_int32), ("kappa", C.c_float), ("scale", C.c_float), ("attack_lr", C.c_float),
                ("init_weight", C.c_float), ("max_weight", C.c_float)]


OBJECT_SIGNATURES = {
    "ifd_object_abi_version": (C.c_int, []),
    "ifd_object_place": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_void_p]),
    "ifd_object_step": (C.c_int, [C.c_void_p, C.POINTER(IfdObjectState), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(IfdObjectDiag), C.c_int, C.c_float, C.c_float,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ifd_object_attack": (C.c_int, [C.c_void_p, C.POINTER(IfdObjectParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
}

# include/ifd_dgcnn.h (the DGCNN victim classifier), versioned on its own
DGCNN_ABI_VERSION = 1
DGCNN_MAX_POINTS, DGCNN_MAX_K = 2048, 32


class IfdDgcnnAux(C.Structure):
    _fields_ = [("idx", C.c_void_p * 4), ("feat", C.c_void_p), ("global_feat", C.c_void_p), ("pred", C.c_void_p)]


DGCNN_SIGNATURES = {
    "ifd_dgcnn_abi_version": (C.c_int, []),
    "ifd_dgcnn_weight_count": (C.c_size_t, []),
    "ifd_dgcnn_create": (C.c_void_p, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int]),
    "ifd_dgcnn_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(IfdDgcnnAux),
                                    C.c_void_p]),
}

# include/ifd_dgcnn_atk.h (input gradients of the DGCNN victim and the FGM family on it), versioned on its own
DGCNN_ATK_ABI_VERSION = 1


class IfdDgcnnGradOut(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("loss", C.c_void_p), ("pred", C.c_void_p), ("idx", C.c_void_p * 4), ("feat", C.c_void_p),
                ("global_feat", C.c_void_p), ("win_pool", C.c_void_p), ("win_edge", C.c_void_p * 4), ("act5", C.c_void_p)]


DGCNN_ATK_SIGNATURES = {
    "ifd_dgcnn_atk_abi_version": (C.c_int, []),
    "ifd_dgcnn_input_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                       C.c_void_p, C.POINTER(IfdDgcnnGradOut), C.c_void_p]),
    "ifd_dgcnn_fgm_update": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                       C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ifd_dgcnn_fgm_attack": (C.c_int, [C.c_void_p, C.POINTER(IfdFgmParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/ifd_pn2.h (the PointNet++ victim classifier), versioned on its own
PN2_ABI_VERSION = 1
PN2_MAX_POINTS = 2048
PN2_NPOINT1, PN2_NSAMPLE1, PN2_NPOINT2, PN2_NSAMPLE2 = 512, 32, 128, 64


class IfdPn2Aux(C.Structure):
    _fields_ = [("fps1", C.c_void_p), ("fps2", C.c_void_p), ("ball1", C.c_void_p), ("ball2", C.c_void_p), ("l1_feat", C.c_void_p),
                ("l2_feat", C.c_void_p), ("global_feat", C.c_void_p), ("pred", C.c_void_p)]


PN2_SIGNATURES = {
    "ifd_pn2_abi_version": (C.c_int, []),
    "ifd_pn2_weight_count": (C.c_size_t, []),
    "ifd_pn2_create": (C.c_void_p, [C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    "ifd_pn2_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(IfdPn2Aux),
                                  C.c_void_p]),
}

# include/ifd_pn2_atk.h (input gradients of the PointNet++ victim and the FGM family on it), versioned on its own
PN2_ATK_ABI_VERSION = 1


class IfdPn2GradOut(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("loss", C.c_void_p), ("pred", C.c_void_p), ("fps1", C.c_void_p), ("fps2", C.c_void_p),
                ("ball1", C.c_void_p), ("ball2", C.c_void_p), ("l1_feat", C.c_void_p), ("l2_feat", C.c_void_p),
                ("global_feat", C.c_void_p), ("win1", C.c_void_p), ("win2", C.c_void_p), ("win3", C.c_void_p), ("act1", C.c_void_p),
                ("act2", C.c_void_p), ("act3", C.c_void_p)]


PN2_ATK_SIGNATURES = {
    "ifd_pn2_atk_abi_version": (C.c_int, []),
    "ifd_pn2_input_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                     C.c_float, C.c_void_p, C.POINTER(IfdPn2GradOut), C.c_void_p]),
    "ifd_pn2_fgm_update": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                     C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ifd_pn2_fgm_attack": (C.c_int, [C.c_void_p, C.POINTER(IfdFgmParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/ifd_pc.h (the PointConv victim classifier), versioned on its own
PC_ABI_VERSION = 1
PC_MAX_POINTS, PC_MIN_POINTS = 2048, 32
PC_NPOINT1, PC_K1, PC_NPOINT2, PC_K2 = 512, 32, 128, 64
PC_CHUNK = 32                        # IFD_PC_CHUNK: most clouds of one chunk of ifd_pc_forward


class IfdPcAux(C.Structure):
    _fields_ = [("fps1", C.c_void_p), ("fps2", C.c_void_p), ("knn1", C.c_void_p), ("knn2", C.c_void_p), ("dens1", C.c_void_p),
                ("dens2", C.c_void_p), ("dens3", C.c_void_p), ("l1_feat", C.c_void_p), ("l2_feat", C.c_void_p),
                ("global_feat", C.c_void_p), ("pred", C.c_void_p)]


PC_SIGNATURES = {
    "ifd_pc_abi_version": (C.c_int, []),
    "ifd_pc_weight_count": (C.c_size_t, []),
    "ifd_pc_create": (C.c_void_p, [C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    "ifd_pc_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(IfdPcAux),
                                 C.c_void_p]),
}

# include/ifd_pc_atk.h (input gradients of the PointConv victim and the FGM family on it), versioned on its own
PC_ATK_ABI_VERSION = 1


class IfdPcGradOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in (
        "logits", "loss", "pred", "fps1", "fps2", "knn1", "knn2", "dens1", "dens2", "dens3", "l1_feat", "l2_feat", "global_feat",
        "dgate1", "dgate2", "dgate3", "wgate1", "wgate2", "wgate3", "mgate1", "mgate2", "mgate3")]


PC_ATK_SIGNATURES = {
    "ifd_pc_atk_abi_version": (C.c_int, []),
    "ifd_pc_input_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                    C.c_float, C.c_void_p, C.POINTER(IfdPcGradOut), C.c_void_p]),
    "ifd_pc_fgm_update": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                    C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ifd_pc_fgm_attack": (C.c_int, [C.c_void_p, C.POINTER(IfdFgmParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/ifd_victim_atk.h (Perturb, kNN and Drop on any of the four victims), versioned on its own
VICTIM_ATK_ABI_VERSION = 1

_P = C.c_void_p
VICTIM_ATK_SIGNATURES = {
    "ifd_victim_atk_abi_version": (C.c_int, []),
    # the step calls: the signatures of ifd_cw_step, ifd_cw_adjust, ifd_knn_step, ifd_knn_project_clip, ifd_drop_step
    "ifd_victim_cw_step": CW_SIGNATURES["ifd_cw_step"],
    "ifd_victim_cw_adjust": CW_SIGNATURES["ifd_cw_adjust"],
    "ifd_victim_knn_step": KNN_SIGNATURES["ifd_knn_step"],
    "ifd_victim_knn_project_clip": KNN_SIGNATURES["ifd_knn_project_clip"],
    "ifd_victim_drop_step": DROP_SIGNATURES["ifd_drop_step"],
    # the loops: fps_start behind n_points
    "ifd_victim_cw_perturb_attack": (C.c_int, [_P, C.POINTER(IfdCwParams), _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "ifd_victim_knn_attack": (C.c_int, [_P, C.POINTER(IfdKnnParams), _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "ifd_victim_drop_attack": (C.c_int, [_P, C.POINTER(IfdDropParams), _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load libifd.so (after torch, so both share one HIP runtime) and bind every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libifd.so is not built (%s). Run `python if-defense_amd/build.py` (needs hipcc); "
            "there is no CPU or PyTorch fallback for the restoration path." % LIB_PATH)
    import torch  # noqa: F401  (loads libamdhip64.so.7 first; libifd binds to the same runtime)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in list(SIGNATURES.items()) + list(DUP_SIGNATURES.items()) + list(CLS_SIGNATURES.items()) + \
            list(ATK_SIGNATURES.items()) + list(CW_SIGNATURES.items()) + list(KNN_SIGNATURES.items()) + list(ADD_SIGNATURES.items()) + \
            list(DROP_SIGNATURES.items()) + list(CLUSTER_SIGNATURES.items()) + list(OBJECT_SIGNATURES.items()) + \
            list(DGCNN_SIGNATURES.items()) + list(DGCNN_ATK_SIGNATURES.items()) + list(PN2_SIGNATURES.items()) + \
            list(PN2_ATK_SIGNATURES.items()) + list(PC_SIGNATURES.items()) + list(PC_ATK_SIGNATURES.items()) + \
            list(VICTIM_ATK_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError if the library lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.ifd_abi_version() != ABI_VERSION:
        raise ImportError("libifd.so ABI %d != binding ABI %d; rebuild" % (lib.ifd_abi_version(), ABI_VERSION))
    if lib.ifd_dup_abi_version() != DUP_ABI_VERSION:
        raise ImportError("libifd.so DUP ABI %d != binding DUP ABI %d; rebuild" % (lib.ifd_dup_abi_version(), DUP_ABI_VERSION))
    if lib.ifd_cls_abi_version() != CLS_ABI_VERSION:
        raise ImportError("libifd.so CLS ABI %d != binding CLS ABI %d; rebuild" % (lib.ifd_cls_abi_version(), CLS_ABI_VERSION))
    if lib.ifd_atk_abi_version() != ATK_ABI_VERSION:
        raise ImportError("libifd.so ATK ABI %d != binding ATK ABI %d; rebuild" % (lib.ifd_atk_abi_version(), ATK_ABI_VERSION))
    if lib.ifd_cw_abi_version() != CW_ABI_VERSION:
        raise ImportError("libifd.so CW ABI %d != binding CW ABI %d; rebuild" % (lib.ifd_cw_abi_version(), CW_ABI_VERSION))
    if lib.ifd_knn_abi_version() != KNN_ABI_VERSION:
        raise ImportError("libifd.so KNN ABI %d != binding KNN ABI %d; rebuild" % (lib.ifd_knn_abi_version(), KNN_ABI_VERSION))
    if lib.ifd_add_abi_version() != ADD_ABI_VERSION:
        raise ImportError("libifd.so ADD ABI %d != binding ADD ABI %d; rebuild" % (lib.ifd_add_abi_version(), ADD_ABI_VERSION))
    if lib.ifd_drop_abi_version() != DROP_ABI_VERSION:
        raise ImportError("libifd.so DROP ABI %d != binding DROP ABI %d; rebuild" % (lib.ifd_drop_abi_version(), DROP_ABI_VERSION))
    if lib.ifd_cluster_abi_version() != CLUSTER_ABI_VERSION:
        raise ImportError("libifd.so CLUSTER ABI %d != binding CLUSTER ABI %d; rebuild" % (lib.ifd_cluster_abi_version(), CLUSTER_ABI_VERSION))
    if lib.ifd_object_abi_version() != OBJECT_ABI_VERSION:
        raise ImportError("libifd.so OBJECT ABI %d != binding OBJECT ABI %d; rebuild" % (lib.ifd_object_abi_version(), OBJECT_ABI_VERSION))
    if lib.ifd_dgcnn_abi_version() != DGCNN_ABI_VERSION:
        raise ImportError("libifd.so DGCNN ABI %d != binding DGCNN ABI %d; rebuild" % (lib.ifd_dgcnn_abi_version(), DGCNN_ABI_VERSION))
    if lib.ifd_dgcnn_atk_abi_version() != DGCNN_ATK_ABI_VERSION:
        raise ImportError("libifd.so DGCNN ATK ABI %d != binding DGCNN ATK ABI %d; rebuild" %
                          (lib.ifd_dgcnn_atk_abi_version(), DGCNN_ATK_ABI_VERSION))
    if lib.ifd_pn2_abi_version() != PN2_ABI_VERSION:
        raise ImportError("libifd.so PN2 ABI %d != binding PN2 ABI %d; rebuild" % (lib.ifd_pn2_abi_version(), PN2_ABI_VERSION))
    if lib.ifd_pn2_atk_abi_version() != PN2_ATK_ABI_VERSION:
        raise ImportError("libifd.so PN2 ATK ABI %d != binding PN2 ATK ABI %d; rebuild" %
                          (lib.ifd_pn2_atk_abi_version(), PN2_ATK_ABI_VERSION))
    if lib.ifd_pc_abi_version() != PC_ABI_VERSION:
        raise ImportError("libifd.so PC ABI %d != binding PC ABI %d; rebuild" % (lib.ifd_pc_abi_version(), PC_ABI_VERSION))
    if lib.ifd_pc_atk_abi_version() != PC_ATK_ABI_VERSION:
        raise ImportError("libifd.so PC ATK ABI %d != binding PC ATK ABI %d; rebuild" %
                          (lib.ifd_pc_atk_abi_version(), PC_ATK_ABI_VERSION))
    if lib.ifd_victim_atk_abi_version() != VICTIM_ATK_ABI_VERSION:
        raise ImportError("libifd.so VICTIM ATK ABI %d != binding VICTIM ATK ABI %d; rebuild" %
                          (lib.ifd_victim_atk_abi_version(), VICTIM_ATK_ABI_VERSION))
    _lib = lib
    return lib
