"""ctypes binding of the C ABI in include/capf.h.  PyTorch is used for device memory and streams
only (tensor.data_ptr(), torch.cuda.current_stream()); no torch type crosses the ABI."""
import ctypes
import math
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

# CAPF_LIB: an alternative build of the same ABI (A/B timing of kernel variants on one GPU box; tools only)
LIB_PATH = os.environ.get("CAPF_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libcapf.so")
HRNET, CPN50 = 0, 1
F32, BF16, F16 = 0, 1, 2      # capf_dtype
PLAN_NO_FUSED_LIFTER, PLAN_NO_WINOGRAD, PLAN_NO_ROW_HALO, PLAN_WINOGRAD_F23_ONLY, PLAN_NO_PWCHAIN, PLAN_NO_WS, PLAN_LIFTER_FP32, PLAN_NO_F32X3, PLAN_F32X3_EXACT, PLAN_NO_F32H2_GEMM, PLAN_NO_UPADD, PLAN_H2_PLANES, PLAN_NO_BNECK, PLAN_NO_BATCHED_REDUCE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192     # capf_plan_flag
PLAN_BF16_F32_STREAM = 32768     # (1 << 14 stays unassigned)
PLAN_BN_BATCH_STATS = 65536      # opt-in: the handle also carries the batch-statistics backbone route (capf_backbone_forward_bn)
PLAN_CPN_PREDICT = 131072        # opt-in, CPN50 (fp32 / bf16): the backbone also runs refine_net.final_predict into the named tensor "heat"
ABI_VERSION = 12       # include/capf.h :: CAPF_ABI_VERSION (checked against capf_abi_version() at load)


class CapfError(RuntimeError):
    pass


def _bf16():
    import torch
    return torch.bfloat16


def _f16():
    import torch
    return torch.float16


_TORCH16 = {2: _bf16, 3: _f16}          # capf_tensor / capf_op_desc dtype code -> torch dtype of a 16-bit tensor
_TORCH16_OF = {BF16: _bf16, F16: _f16}  # capf_dtype -> the same


class CapfConfig(ctypes.Structure):
    _fields_ = [
        ("backbone", c_int32), ("hr_channels", c_int32 * 4), ("hr_modules", c_int32 * 3), ("hr_blocks", c_int32),
        ("base_dim", c_int32), ("embed_dim_ratio", c_int32), ("levels", c_int32), ("num_joints", c_int32),
        ("num_heads", c_int32), ("deform_heads", c_int32), ("deform_samples", c_int32), ("context_blocks", c_int32),
        ("compute_dtype", c_int32), ("max_batch", c_int32), ("height", c_int32), ("width", c_int32),
        ("training", c_int32), ("plan_flags", c_int32), ("depth", c_int32),
    ]


class OpDesc(ctypes.Structure):
    """mirrors include/capf.h :: capf_op_desc"""
    _fields_ = [(k, c_int32) for k in ("kind", "backbone", "conv", "Cin", "H", "W", "Cout", "Ho", "Wo", "ks", "stride", "pad", "act",
                                       "in_dtype", "out_dtype", "mfma_bf16", "n_in")] + [("shift", c_int32 * 4)] + \
               [(k, c_int32) for k in ("relu", "p_weight", "p_bn_weight", "has_residual", "checkpoint", "rows_per_frame", "p_bias",
                                       "p_ln_weight", "p_ln_bias")] + [("eps", c_float), ("attn", c_int32 * 4), ("maps", (c_int64 * 4) * 3),
                                                                         ("up_H", c_int32), ("up_W", c_int32)]


class ConvDesc(ctypes.Structure):
    """mirrors include/capf.h :: capf_conv_desc"""
    _fields_ = [("x", ctypes.c_void_p), ("w_packed", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                ("residual", ctypes.c_void_p), ("y", ctypes.c_void_p)] + \
               [(k, ctypes.c_int32) for k in ("B", "H", "W", "Cin", "Cout", "ks", "stride", "act")]


class OptimReport(ctypes.Structure):
    """mirrors include/capf.h :: capf_optim_report (the head of the guarded AdamW step's control block)"""
    _fields_ = [(k, c_int64) for k in ("steps_taken", "steps_skipped", "nonfinite_losses", "grad_nonfinite")] + \
               [(k, c_double) for k in ("grad_sumsq", "grad_norm", "clip_coef", "loss_sum", "loss_rows")]


class OptimSegment(ctypes.Structure):
    """mirrors include/capf.h :: capf_optim_segment"""
    _fields_ = [("begin", c_int64), ("end", c_int64), ("lr", c_float), ("weight_decay", c_float)]


OPTIM_MAX_SEGMENTS = 64       # include/capf.h :: CAPF_OPTIM_MAX_SEGMENTS

# ---- the C ABI, declared once: one row per function of include/capf.h, in the header's order, name -> (restype, argtypes).  load_library()
# applies the rows; tests/test_abi.py holds every row, the struct mirrors above and the constants to the header.
# A pointer whose pointee is a scalar or a mirrored struct that the HOST reads or writes is POINTER(T); a device pointer, a stream, a void*
# and an opaque handle are c_void_p, and so is the address of a numpy buffer (the JPEG coefficient and matrix arguments).
I, I64, Z, F, S = c_int, c_int64, c_size_t, c_float, c_char_p
H = P = c_void_p                                # the handle; a device pointer / stream / void*
pP, pS = POINTER(c_void_p), POINTER(c_char_p)
pI32, pI64, pZ, pF, pD = POINTER(c_int32), POINTER(c_int64), POINTER(c_size_t), POINTER(c_float), POINTER(c_double)
D = POINTER(ConvDesc)
FOLD = [P, P, P, P, P, P, F, P, P]              # the head of every fold-and-pack entry: stream, w, gamma, beta, mean, var, eps, w_packed, bias
RUN = [H, P, P, P, P, I, P]                     # capf_forward's arguments: handle, stream, images, k2d, kcrop_inout, batch, out

PROTOTYPES = {
    "capf_create": (I, [POINTER(CapfConfig), I, POINTER(H)]),
    "capf_destroy": (None, [H]),
    "capf_max_batch": (I, [H]),
    "capf_last_error": (S, [H]),
    "capf_version": (S, []),
    "capf_abi_version": (I, []),
    "capf_num_params": (I, [H]),
    "capf_param_info": (I, [H, I, pS, pI64, pI32, pI32]),
    "capf_set_param": (I, [H, S, P, pI64, I]),
    "capf_params_changed": (I, [H, P]),
    "capf_lifter_params_changed": (I, [H, P]),
    "capf_workspace_bytes": (Z, [H, I]),
    "capf_set_workspace": (I, [H, P, Z]),
    "capf_forward": (I, RUN),
    "capf_backbone_forward": (I, [H, P, P, I]),
    "capf_backbone_forward_bn": (I, [H, P, P, I, F]),
    "capf_forward_train": (I, RUN + [P]),
    "capf_backward": (I, [H, P, P, I, P, P]),
    "capf_train_generation": (I64, [H]),
    "capf_grad_elems": (I64, [H]),
    "capf_grad_info": (I, [H, I, pI64]),
    "capf_train_h2_matrices": (I, [H]),
    "capf_mpjpe": (I, [P, P, P, I, P, P, F]),
    "capf_mpjpe_nd": (I, [P, P, P, I, I, P, P, F]),
    "capf_adamw_step": (I, [P, P, P, P, P, I64, F, F, F, F, F, I, F]),
    "capf_optim_ctrl_bytes": (Z, []),
    "capf_optim_ctrl_init": (I, [P, P, I64]),
    "capf_grad_sumsq": (I, [P, P, I64, F, P]),
    "capf_adamw_step_guarded": (I, [P, P, P, P, P, I64, POINTER(OptimSegment), I, F, F, F, F, F, I64, P, I, P]),
    "capf_lifter_forward": (I, [H, P, P, P, I, P]),
    "capf_set_features": (I, [H, P, pP, I]),
    "capf_lifter_forward_train": (I, [H, P, P, P, I, P, P]),
    "capf_backward_maps": (I, [H, P, P, I, P, P, pP]),
    "capf_set_map_grad_mode": (I, [H, I]),
    "capf_map_grad_mode": (I, [H]),
    "capf_backward_points": (I, [H, P, P, I, P, P, pP, P, P]),
    "capf_set_lanes": (I, [H, I]),
    "capf_set_debug": (I, [H, I]),
    "capf_tensor": (I, [H, S, pP, pI64, pI32]),
    "capf_forward_profile_variants": (I, [H, pI32, I]),
    "capf_forward_stats": (I, [H, I, pI64, pD]),
    "capf_op_pack_conv": (I, FOLD + [I, I, I]),
    "capf_op_conv": (I, [P] * 6 + [I] * 8),
    "capf_op_conv_group": (I, [P, I, D]),
    "capf_op_pack_conv_wino": (I, FOLD + [I, I, I]),
    "capf_op_conv_wino": (I, [P] * 6 + [I] * 7),
    "capf_op_conv_wino_group": (I, [P, I, D, I]),
    "capf_op_linear": (I, [P] * 6 + [I] * 4),
    "capf_op_bn_stats_scratch_bytes": (Z, [I64, I]),
    "capf_op_bn_stats": (I, [P, P, I64, I, P, P, F, F, P, P, P, P, P, Z]),
    "capf_op_bn_apply": (I, [P] * 6 + [I64, I, I]),
    "capf_op_bilinear_corners": (I, [P, P, I, I, I, I, P, P]),
    "capf_op_pack_conv_bf16": (I, FOLD + [I, I, I]),
    "capf_op_conv_bf16": (I, [P] * 6 + [I] * 8),
    "capf_op_conv_bf16_rh_width": (I, [I]),
    "capf_op_pack_conv_bf16_rh": (I, FOLD + [I, I]),
    "capf_op_conv_bf16_rh": (I, [P] * 6 + [I] * 6),
    "capf_op_conv_bf16_ws_pack_elems": (I64, [I, I]),
    "capf_op_pack_conv_bf16_ws": (I, FOLD + [I, I]),
    "capf_op_conv_bf16_ws_group": (I, [P, I, D]),
    "capf_op_conv_f32x3_pack_elems": (I64, [I, I]),
    "capf_op_pack_conv_f32x3": (I, FOLD + [I, I]),
    "capf_op_conv_f32x3_group": (I, [P, I, D]),
    "capf_op_conv_f32h2_pack_elems": (I64, [I, I]),
    "capf_op_pack_conv_f32h2": (I, FOLD + [I, I]),
    "capf_op_conv_f32h2_group": (I, [P, I, D]),
    "capf_op_conv_f32h2_tiles": (I, [I, I, I, pI32]),
    "capf_op_conv_f32h2_planes": (I, [P, D, P, P]),
    "capf_op_f32h2_gemm_pack_elems": (I64, [I, I]),
    "capf_op_pack_f32h2_gemm": (I, FOLD + [I, I, I, I]),
    "capf_op_conv_f32h2g": (I, [P] * 6 + [I] * 8),
    "capf_op_conv_f32h2g_group": (I, [P, I, D]),
    "capf_op_linear_f32h2g": (I, [P] * 6 + [I] * 4),
    "capf_op_wgrad": (I, [P, P, P, I, I, I, P, I]),
    "capf_op_linear_ln_f32h2g": (I, [P, P, P, P, F, P, P, P, P] + [I] * 4),
    "capf_op_conv_bf16_group": (I, [P, I, D, pP, pI32]),
    "capf_op_linear_bf16": (I, [P] * 6 + [I] * 4),
    "capf_op_pack_conv_16": (I, FOLD + [I] * 5),
    "capf_op_conv_16": (I, [P] * 6 + [I] * 9),
    "capf_op_conv_16_group": (I, [P, I, D, pP, pI32, I]),
    "capf_op_conv_16_ws_group": (I, [P, I, D, I]),
    "capf_op_linear_16": (I, [P] * 6 + [I] * 5),
    "capf_op_bneck_16": (I, [P, P, pP, pP, P, P, P, P] + [I] * 5),
    "capf_debug_f16_round": (I, [P, P, I]),
    "capf_preprocess": (I, [P, P, I, I, I, pF, pF, I] + [P] * 7),
    "capf_fliptest_fuse": (I, [P, P, I, P]),
    "capf_forward_u8": (I, [H, P, P, pF, pF, I, P, P, I, P]),
    "capf_backbone_forward_u8": (I, [H, P, P, pF, pF, I, I]),
    "capf_forward_train_u8": (I, [H, P, P, pF, pF, I, P, P, I, P, P]),
    "capf_preprocess_points": (I, [P, I, I] + [P] * 6),
    "capf_input_rule_host": (I, [P, I, I, pF, pF, P]),
    "capf_op_conv_u8": (I, [P] * 5 + [I] * 8 + [pF, pF, I]),
    "capf_op_conv_u8_kernel_name": (S, [I] * 8),
    "capf_op_conv_stem_kernel_name": (S, [I] * 7),
    "capf_fliptest_fuse_swap": (I, [P, P, I, I, pI32, P]),
    "capf_pose_errors": (I, [P, P, P, I, I, P, P]),
    "capf_segment_sums": (I, [P, P, P, P, I, I, P, P]),
    "capf_keypoints_loss": (I, [P, I, P, P, P, I, I, F, P, P]),
    "capf_keypoints_l2_loss": (I, [P, P, P, P, I, I, P, P, F]),
    "capf_limb_length_errors": (I, [P, P, P, I, I, pI32, I, P, P, F]),
    "capf_limb_length_sums": (I, [P, P, P, I, I, I, P, P]),
    "capf_uncertainty_loss": (I, [P, P, P, I, I, pP, pI32, I, P, P, pP, F]),
    "capf_kp_head_scratch_bytes": (Z, [I] * 6),
    "capf_kp_head_forward": (I, [P, P, I, P, P] + [I] * 6 + [F, pF, P, P, P, P, P, P, Z]),
    "capf_kp_head_backward": (I, [P, P, P, P, I, P, P] + [I] * 6 + [F, pF, P, P, P, P, I, P, Z]),
    "capf_kp_head_pair_scratch_bytes": (Z, [I] * 5),
    "capf_kp_head_forward_pair": (I, [P, P, I, P, P] + [I] * 6 + [F, pI32, I, pF, P, F, P, P, P, P, P, Z]),
    "capf_kp_heatmap_loss_scratch_bytes": (Z, [I] * 6),
    "capf_kp_heatmap_loss": (I, [P, P, I, P, P] + [I] * 5 + [P, P, pF, F, I, I, F, P, P, P, P, P, I, P, Z]),
    "capf_cpn_decode_taps": (None, [pD]),
    "capf_cpn_decode_lds_bytes": (Z, [I, I]),
    "capf_cpn_decode": (I, [P, P] + [I] * 6 + [pF, P, P, P, P, P]),
    "capf_cpn_decode_pair": (I, [P, P] + [I] * 6 + [pI32, pF, P, F, P, P, P, P, P]),
    "capf_pck_counts": (I, [P, P, P, I, I, I, c_double, P, I, P, P, P]),
    "capf_pck2d_counts": (I, [P, P, P, I, I, P, P, pD, I, I, P, I, P, P, P]),
    "capf_jpeg_info": (I, [S, Z, pI32, pI32, pI32, pI32, pI32, pZ]),
    "capf_jpeg_coefficients": (I, [S, Z, P, Z]),
    "capf_jpeg_decode": (I, [P, S, Z, P, Z, P, Z]),
    "capf_jpeg_batch_info": (I, [I, P, pZ, I, pI32, pZ]),
    "capf_jpeg_decode_batch": (I, [P, I, P, pZ, P, pZ, P, P, Z, P, I]),
    "capf_jpeg_coefficients_subseq": (I, [S, Z, P, Z, I]),
    "capf_jpeg_crop_rect": (I, [I, I, I, I, pD, I, I, pI32, pI32]),
    "capf_jpeg_crop_batch_info": (I, [I, P, pZ, P, I, I, I, pI32, pZ]),
    "capf_jpeg_decode_crop_batch": (I, [P, I, P, pZ, P, I, I, P, P, Z, P, I]),
    "capf_affine_from_center_scale": (I, [pD, pD, I, I, pD]),
    "capf_warp_affine": (I, [P, P, P, P, I, I, I, P]),
    "capf_erase_scratch_bytes": (Z, [I, I]),
    "capf_erase_patches": (I, [P, P, I, I, I, P, P, I, I, I, P, P, Z]),
    "capf_num_ops": (I, [H]),
    "capf_op_info": (I, [H, I, I, pS, pS, pD]),
    "capf_op_executed_flops": (I, [H, I, I, pD]),
    "capf_op_bytes": (I, [H, I, I, pD]),
    "capf_op_schedule": (I, [H, I, pI32, pI32, pI32, pI32, pI32]),
    "capf_op_stream_class": (I, [H, I, I]),
    "capf_forward_prefix": (I, RUN + [I]),
    "capf_op_describe": (I, [H, I, POINTER(OpDesc)]),
    "capf_op_describe_sized": (I, [H, I, P, Z]),
    "capf_op_tensor": (I, [H, I, I, pP]),
    "capf_op_h2_planes": (I, [H, I, I, pP, pI32]),
    "capf_forward_profile": (I, RUN + [pF, I]),
    "capf_forward_profile_launches": (I, RUN + [pF, pI32, I]),
}
EXPORTS = list(PROTOTYPES)    # every symbol include/capf.h declares

_lib = None


def load_library():
    """Load libcapf.so; fail loudly (no CPU / eager fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64/libhsa-runtime64: it must be loaded FIRST so that libcapf.so
    # binds to the same HIP runtime (two runtimes in one process do not share devices or streams).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise CapfError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
                        "(or make -C contextaware-poseformer_amd/csrc); there is no fallback path")
    lib = ctypes.CDLL(LIB_PATH)
    # structs cross this boundary (CapfConfig, ConvDesc, OpDesc): a library built from another revision of capf.h must not be driven
    # with this file's layouts
    abi = lib.capf_abi_version()
    if abi != ABI_VERSION:
        raise CapfError(f"{LIB_PATH} implements ABI revision {abi}, this binding expects {ABI_VERSION}: rebuild the library")
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


PARAM_KINDS = {0: "conv_w", 1: "bn_w", 2: "bn_b", 3: "bn_mean", 4: "bn_var", 5: "bn_nbt", 6: "lin_w", 7: "lin_b",
               8: "ln_w", 9: "ln_b", 10: "raw"}


def _p(t):
    """a tensor's device pointer for the C ABI; None -> a null pointer"""
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


class Engine:
    """One native handle.  device=None -> plan-only (schema / workspace queries, no GPU)."""

    def __init__(self, cfg: CapfConfig, device=None):
        self.lib = load_library()
        self.cfg = cfg
        self.h = c_void_p()
        rc = self.lib.capf_create(byref(cfg), -1 if device is None else int(device), byref(self.h))
        if rc != 0:
            raise CapfError(f"capf_create failed ({rc}): {self.lib.capf_last_error(None).decode()}")
        self.device = device
        self._ws = None
        self._ws_batch = 0
        self._bound = {}

    def close(self):
        if getattr(self, "h", None):
            self.lib.capf_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc, what):
        if rc < 0:
            raise CapfError(f"{what} failed ({rc}): {self.lib.capf_last_error(self.h).decode()}")
        return rc

    # ---- schema
    def schema(self):
        """[(name, shape tuple, kind str)] == the reference's state_dict (incl. BN buffers)."""
        out = []
        name, shape, nd, kind = c_char_p(), (c_int64 * 4)(), c_int(), c_int()
        for i in range(self.lib.capf_num_params(self.h)):
            self._check(self.lib.capf_param_info(self.h, i, byref(name), shape, byref(nd), byref(kind)), "param_info")
            out.append((name.value.decode(), tuple(shape[j] for j in range(nd.value)), PARAM_KINDS[kind.value]))
        return out

    # ---- parameters
    def bind_state(self, named_tensors, stream=0):
        """Borrow device pointers for every schema entry from {name: cuda fp32 tensor}; fold/pack."""
        import torch
        for name, shape, kind in self.schema():
            if kind == "bn_nbt":
                continue
            t = named_tensors[name]
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise CapfError(f"{name}: need a contiguous fp32 CUDA tensor, got {t.dtype} {t.device}")
            if self._bound.get(name) == t.data_ptr():
                continue
            shp = (c_int64 * 4)(*(list(t.shape) + [0] * (4 - t.dim())))
            self._check(self.lib.capf_set_param(self.h, name.encode(), c_void_p(t.data_ptr()), shp, t.dim()),
                        f"set_param({name})")
            self._bound[name] = t.data_ptr()
        self.params_changed(stream)

    def params_changed(self, stream=0):
        self._check(self.lib.capf_params_changed(self.h, c_void_p(stream)), "params_changed")

    def lifter_params_changed(self, stream=0):
        self._check(self.lib.capf_lifter_params_changed(self.h, c_void_p(stream)), "lifter_params_changed")

    # ---- workspace
    def workspace_bytes(self, batch):
        return self.lib.capf_workspace_bytes(self.h, batch)

    def ensure_workspace(self, batch):
        import torch
        if self._ws is None or batch > self._ws_batch:
            nbytes = self.workspace_bytes(batch)
            self._ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=f"cuda:{self.device}")
            self._ws_batch = batch
            self._check(self.lib.capf_set_workspace(self.h, c_void_p(self._ws.data_ptr()), nbytes), "set_workspace")

    # ---- hot path
    def _run(self, entry, batch, stream, *args):
        """capf_<entry>(handle, stream, *args) with the workspace sized for `batch` frames first (None: a backward, which runs in the
        workspace of its forward); a negative status raises "<entry> failed (rc): message"."""
        if batch is not None:
            self.ensure_workspace(batch)
        self._check(getattr(self.lib, "capf_" + entry)(self.h, c_void_p(stream), *args), entry)

    def forward(self, images, k2d, kcrop, out, stream):
        B = images.shape[0]
        self._run("forward", B, stream, _p(images), _p(k2d), _p(kcrop), B, _p(out))

    # ---- the same from uint8 BGR crops [Bsrc,H,W,3] (capf_forward_u8 ...): mode 0 as is, 1 mirrored, 2 flip-test pair (2 * Bsrc engine frames);
    # mean / std: (c_float * 3) arrays (input_constants), std None = mean only.  k2d / kcrop / out hold the ENGINE frames
    @staticmethod
    def _u8_batch(images_u8, mode):
        return images_u8.shape[0] * (2 if mode == 2 else 1)

    def forward_u8(self, images_u8, mean, std, mode, k2d, kcrop, out, stream):
        B = self._u8_batch(images_u8, mode)
        self._run("forward_u8", B, stream, _p(images_u8), mean, std, int(mode), _p(k2d), _p(kcrop), B, _p(out))

    def backbone_forward_u8(self, images_u8, mean, std, mode, stream):
        B = self._u8_batch(images_u8, mode)
        self._run("backbone_forward_u8", B, stream, _p(images_u8), mean, std, int(mode), B)

    def forward_train_u8(self, images_u8, mean, std, mode, k2d, kcrop, out, stream, masks=None):
        B = self._u8_batch(images_u8, mode)
        self._run("forward_train_u8", B, stream, _p(images_u8), mean, std, int(mode), _p(k2d), _p(kcrop), B, _p(out), _p(masks))

    # ---- training step
    def grad_layout(self):
        """{parameter name: (offset, numel)} inside the flat lifter gradient; total element count."""
        out, off = {}, c_int64()
        for i, (name, shape, kind) in enumerate(self.schema()):
            self._check(self.lib.capf_grad_info(self.h, i, byref(off)), "grad_info")
            if off.value >= 0:
                n = 1
                for d in shape:
                    n *= d
                out[name] = (off.value, n)
        return out, self.lib.capf_grad_elems(self.h)

    def grad_layout_cached(self):
        if not hasattr(self, "_grad_layout"):
            self._grad_layout = self.grad_layout()
        return self._grad_layout

    def forward_train(self, images, k2d, kcrop, out, stream, masks=None):
        B = images.shape[0]
        self._run("forward_train", B, stream, _p(images), _p(k2d), _p(kcrop), B, _p(out), _p(masks))

    def train_generation(self):
        return self.lib.capf_train_generation(self.h)

    def max_batch(self):
        return self.lib.capf_max_batch(self.h)

    def backward(self, grad_out, flat_grad, stream, masks=None):
        self._run("backward", None, stream, _p(grad_out), grad_out.shape[0], _p(flat_grad), _p(masks))

    # ---- the lifter on caller-supplied context maps (capf_set_features / capf_lifter_forward_train / capf_backward_maps)
    def feature_shapes(self):
        """[(H_l, W_l, C_l)] of the four context maps feat0..3 (NHWC) of this plan."""
        if not hasattr(self, "_feature_shapes"):
            shape, nd, out = (c_int64 * 4)(), c_int(), []
            for l in range(4):
                self._check(self.lib.capf_tensor(self.h, f"feat{l}".encode(), None, shape, byref(nd)), f"tensor(feat{l})")
                out.append((shape[1], shape[2], shape[3]))
            self._feature_shapes = out
        return self._feature_shapes

    def tensor_shape(self, name):
        """(dtype code, per-frame shape) of a named tensor of this plan -- capf_tensor's return value (0 fp32, 1 int32, 2 bf16, 3 fp16) and
        its shape without the batch; works on a plan-only handle.  An unknown name raises ("heat" exists under PLAN_CPN_PREDICT only)."""
        shape, nd = (c_int64 * 4)(), c_int()
        rc = self._check(self.lib.capf_tensor(self.h, name.encode(), None, shape, byref(nd)), f"tensor({name})")
        return rc, tuple(shape[i] for i in range(1, nd.value))

    @staticmethod
    def _ptrs4(tensors):
        return (c_void_p * 4)(*[t.data_ptr() for t in tensors])

    def set_features(self, feats_nhwc, stream):
        """Copy four contiguous fp32 NHWC maps [B, H_l, W_l, C_l] into the workspace's feat0..3."""
        B = feats_nhwc[0].shape[0]
        self._run("set_features", B, stream, self._ptrs4(feats_nhwc), B)

    def lifter_forward_train(self, k2d, kcrop, out, stream, masks=None):
        B = k2d.shape[0]
        self._run("lifter_forward_train", B, stream, _p(k2d), _p(kcrop), B, _p(out), _p(masks))

    def backward_maps(self, grad_out, flat_grad, dfeat_nhwc, stream, masks=None):
        """capf_backward plus the gradient w.r.t. the context maps, written into four contiguous fp32 NHWC tensors."""
        self._run("backward_maps", None, stream, _p(grad_out), grad_out.shape[0], _p(flat_grad), _p(masks), self._ptrs4(dfeat_nhwc))

    def backward_points(self, grad_out, flat_grad, stream, masks=None, dfeat_nhwc=None, dk2d=None, dref=None):
        """capf_backward plus any of: the map gradient (four contiguous fp32 NHWC tensors, as backward_maps), dk2d and dref (contiguous
        fp32 [B, J, 2]; dref is w.r.t. the NORMALISED crop keypoints).  None: that output is not computed."""
        self._run("backward_points", None, stream, _p(grad_out), grad_out.shape[0], _p(flat_grad), _p(masks),
                  self._ptrs4(dfeat_nhwc) if dfeat_nhwc is not None else None, _p(dk2d), _p(dref))

    def set_map_grad_mode(self, mode):
        """How capf_backward_maps sums the map gradient: 0 fp32 atomic adds (default), 1 the ordered, bit-reproducible sum."""
        self._check(self.lib.capf_set_map_grad_mode(self.h, int(mode)), "set_map_grad_mode")

    def map_grad_mode(self):
        return self.lib.capf_map_grad_mode(self.h)

    def backbone_forward(self, images, stream):
        B = images.shape[0]
        self._run("backbone_forward", B, stream, _p(images), B)

    def backbone_forward_bn(self, images, stream, momentum=0.1):
        """capf_backbone_forward_bn: the backbone with batch statistics (a PLAN_BN_BATCH_STATS handle); the bound running_mean /
        running_var tensors are updated in place."""
        B = images.shape[0]
        self._run("backbone_forward_bn", B, stream, _p(images), B, float(momentum))

    def lifter_forward(self, k2d, kcrop, out, stream):
        B = k2d.shape[0]
        self._run("lifter_forward", B, stream, _p(k2d), _p(kcrop), B, _p(out))

    def set_lanes(self, on):
        self._check(self.lib.capf_set_lanes(self.h, int(on)), "set_lanes")

    def set_debug(self, on):
        self._check(self.lib.capf_set_debug(self.h, int(on)), "set_debug")

    def _ws_view(self, ptr, n, code):
        """The n elements at device address `ptr` inside the workspace as a flat view (no copy) of the dtype that `code` names (capf_tensor's
        convention: 0 fp32, 1 int32, 2 bf16, 3 fp16)."""
        import torch
        off = (ptr - self._ws.data_ptr()) // 4
        if code in (2, 3):  # bf16 / fp16 tensor: two elements per float slot
            return self._ws[off:off + (n + 1) // 2].view(_TORCH16[code]())[:n]
        flat = self._ws[off:off + n]
        return flat.view(torch.int32) if code == 1 else flat

    def tensor(self, name):
        """Copy of a named intermediate of the last forward (torch tensor on the device)."""
        ptr, shape, nd = c_void_p(), (c_int64 * 4)(), c_int()
        rc = self._check(self.lib.capf_tensor(self.h, name.encode(), byref(ptr), shape, byref(nd)), f"tensor({name})")
        shp = [shape[i] for i in range(nd.value)]
        return self._ws_view(ptr.value, math.prod(shp), rc).view(*shp).clone()

    def tensor_view(self, name, batch):
        """A named intermediate of the last forward of `batch` frames as a VIEW into the workspace (no copy; fp32 / bf16 / fp16 names only):
        valid until the next run on this handle overwrites it.  The keypoint head reads feat0 through it."""
        ptr, shape, nd = c_void_p(), (c_int64 * 4)(), c_int()
        rc = self._check(self.lib.capf_tensor(self.h, name.encode(), byref(ptr), shape, byref(nd)), f"tensor({name})")
        if rc == 1:
            raise CapfError(f"tensor_view({name}): an int32 tensor has no floating-point view")
        shp = [shape[i] for i in range(nd.value)]
        if shp[0] != batch:
            raise CapfError(f"tensor_view({name}): the workspace holds {shp[0]} frames, not {batch}")
        return self._ws_view(ptr.value, math.prod(shp), rc).view(*shp)

    def op_table(self, batch):
        """[(op name, kernel name, algorithmic flops at `batch`)] in launch order."""
        name, kern, fl = c_char_p(), c_char_p(), c_double()
        out = []
        for i in range(self.lib.capf_num_ops(self.h)):
            self._check(self.lib.capf_op_info(self.h, i, batch, byref(name), byref(kern), byref(fl)), "op_info")
            out.append((name.value.decode(), kern.value.decode(), fl.value))
        return out

    def op_bytes(self, batch):
        """algorithmic HBM bytes per op at `batch` (capf_op_bytes), in launch order"""
        b, out = c_double(), []
        for i in range(self.lib.capf_num_ops(self.h)):
            self._check(self.lib.capf_op_bytes(self.h, i, batch, byref(b)), "op_bytes")
            out.append(b.value)
        return out

    def op_executed_flops(self, batch):
        """FLOPs the matrix pipe executes per op at `batch` (capf_op_executed_flops: Winograd ops count 1/2 or 2/3), launch order"""
        f, out = c_double(), []
        for i in range(self.lib.capf_num_ops(self.h)):
            self._check(self.lib.capf_op_executed_flops(self.h, i, batch, byref(f)), "op_executed_flops")
            out.append(f.value)
        return out

    # ---- layer-wise parity aids (capf_forward_prefix / capf_op_describe / capf_op_tensor)
    def forward_prefix(self, images, n_ops, stream, k2d=None, kcrop=None, out=None):
        B = images.shape[0]
        self._prefix_images = images
        self._run("forward_prefix", B, stream, _p(images), _p(k2d), _p(kcrop), B, _p(out), int(n_ops))

    def op_describe(self, index):
        d = OpDesc()
        self._check(self.lib.capf_op_describe_sized(self.h, index, byref(d), ctypes.sizeof(d)), "op_describe")
        return d

    def op_tensor(self, index, slot, shape, dtype_code):
        """View (no copy) of one operand of op `index` after a forward_prefix: slot 0..3 inputs, 4 residual, 5 output, 6 the output's bf16
        shadow (PLAN_BF16_F32_STREAM); shape = full [B, ...] shape, dtype_code 0 fp32 / 2 bf16 / 3 fp16."""
        ptr = c_void_p()
        self._check(self.lib.capf_op_tensor(self.h, index, slot, byref(ptr)), f"op_tensor({index}, {slot})")
        img = getattr(self, "_prefix_images", None)
        if img is not None and ptr.value == img.data_ptr():
            return img.view(*shape)
        return self._ws_view(ptr.value, math.prod(shape), dtype_code).view(*shape)

    def op_h2_planes(self, index, batch):
        """(role, exps [tiles, C / 16] int32 view, tile_pixels) of op `index` at this batch: role 0 = plain fp32 tensors, 1 = its output holds split
        fp16 planes, 2 = its input does (capf_op_h2_planes); C = the planes tensor's channels."""
        ptr, tp = c_void_p(), c_int(0)
        role = self.lib.capf_op_h2_planes(self.h, index, batch, byref(ptr), byref(tp))
        if role <= 0:
            return 0, None, 0
        d = self.op_describe(index)
        C = d.Cout if role == 1 else d.Cin
        tiles = self.lib.capf_op_conv_f32h2_tiles(batch, d.H, d.W, None)
        return role, self._ws_view(ptr.value, tiles * (C // 16), 1).view(tiles, C // 16), tp.value

    def op_tensor_fp32(self, index, slot, shape, dtype_code):
        """op_tensor, with a planes tensor (a BasicBlock's conv1 -> conv2 operand where both run the two-fp16-piece tile) decoded to the fp32 values
        it stands for."""
        t = self.op_tensor(index, slot, shape, dtype_code)
        role, exps, tp = self.op_h2_planes(index, shape[0])
        if (role == 1 and slot == 5) or (role == 2 and slot == 0):
            return planes_to_fp32(t, exps, tp)
        return t

    def forward_profile(self, images, k2d, kcrop, out, stream):
        """One forward with a HIP event pair around every launch (on `stream`); returns ms per op.
        Synchronises the stream — measurement aid for bench.py, not the product path."""
        B = images.shape[0]
        n = self.lib.capf_num_ops(self.h)
        ms = (c_float * n)()
        self._run("forward_profile", B, stream, _p(images), _p(k2d), _p(kcrop), B, _p(out), ms, n)
        return list(ms)

    def op_schedule(self):
        """[(region, level, lane, reads, writes)] per op: see capf_op_schedule."""
        out = []
        for i in range(self.lib.capf_num_ops(self.h)):
            rg, lv, ln = c_int32(), c_int32(), c_int32()
            rd, wr = (c_int32 * 5)(), (c_int32 * 6)()
            self._check(self.lib.capf_op_schedule(self.h, i, byref(rg), byref(lv), byref(ln), rd, wr), "op_schedule")
            out.append((rg.value, lv.value, ln.value, [v for v in rd if v != -1], [v for v in wr if v != -1]))
        return out

    def forward_profile_launches(self, images, k2d, kcrop, out, stream):
        """One forward of the product schedule with an event pair around every LAUNCH (grouped launches
        included); returns (ms per op, leader per op): see capf_forward_profile_launches."""
        B = images.shape[0]
        n = self.lib.capf_num_ops(self.h)
        ms = (c_float * n)()
        leader = (c_int32 * n)()
        self._run("forward_profile_launches", B, stream, _p(images), _p(k2d), _p(kcrop), B, _p(out), ms, leader, n)
        return list(ms), list(leader)

    def op_stream_classes(self, batch):
        """Per op at `batch` under the current set_lanes mode: 0 the caller's stream, 1 a side lane's stream (mode 1) or the side chain's
        (mode 3, batch 16..128): see capf_op_stream_class."""
        return [self._check(self.lib.capf_op_stream_class(self.h, i, batch), "op_stream_class") for i in range(self.lib.capf_num_ops(self.h))]

    def profile_variants(self):
        """After forward_profile_launches: the device kernel of every grouped bf16 launch and of every 2-D halo tile launch (3), by leader op
        (-1 elsewhere)."""
        n = self.lib.capf_num_ops(self.h)
        v = (c_int32 * n)()
        self._check(self.lib.capf_forward_profile_variants(self.h, v, n), "forward_profile_variants")
        return list(v)

    def stats(self, batch):
        n, f = c_int64(), c_double()
        self._check(self.lib.capf_forward_stats(self.h, batch, byref(n), byref(f)), "forward_stats")
        return n.value, f.value


# ---- stateless operators (op-level tests / micro-benchmarks) ---------------------------------------
def _stream(t):
    import torch
    return c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _call(entry, *args):
    """lib.<entry>(*args); a non-zero status raises CapfError"""
    rc = getattr(load_library(), entry)(*args)
    if rc:
        raise CapfError(f"{entry} failed ({rc})")


def _out_hw(H, W, ks, stride):
    """output size of a conv with padding ks // 2"""
    pad = ks // 2
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def _conv_out(d, x, wp, bias, residual, cout, ks=3, stride=1, act=0, bf16=False, dtype=None):
    """Allocate the output [B, Ho, Wo, cout] (fp32, or bf16, or `dtype`) of a conv of NHWC x and describe the conv in the ConvDesc d; -> output."""
    import torch
    B, H, W, ci = x.shape
    y = torch.empty(B, *_out_hw(H, W, ks, stride), cout, device=x.device, dtype=dtype or (torch.bfloat16 if bf16 else torch.float32))
    d.x, d.w_packed, d.bias, d.residual, d.y = (t.data_ptr() if t is not None else None for t in (x, wp, bias, residual, y))
    d.B, d.H, d.W, d.Cin, d.Cout, d.ks, d.stride, d.act = B, H, W, ci, cout, ks, stride, act
    return y


def _conv_descs(problems, bf16=False, dtype=None):
    """problems: (x, wp, bias, residual, cout, ks, stride, act) each -> (ConvDesc array, outputs)"""
    descs = (ConvDesc * len(problems))()
    return descs, [_conv_out(d, *p, bf16=bf16, dtype=dtype) for d, p in zip(descs, problems)]


def _pack(entry, w, bn, eps, wp_shape, wp_dtype, *dims, bias="empty"):
    """BatchNorm-folding weight pack: allocate the packed weights and the fp32 bias [Cout] (torch.<bias>; None: no bias), run lib.<entry>."""
    import torch
    wp = torch.empty(wp_shape, device=w.device, dtype=wp_dtype)
    b_out = getattr(torch, bias)(w.shape[0], device=w.device) if bias else None
    g, b, m, v = bn if bn is not None else (None, None, None, None)
    _call(entry, _stream(w), _p(w.contiguous()), _p(g), _p(b), _p(m), _p(v), eps, _p(wp), _p(b_out), *dims)
    return wp, b_out


def pack_conv(w, bn=None, eps=1e-5):
    """w [Cout,Cin,k,k] cuda fp32; bn = (gamma, beta, mean, var) or None -> (w_packed [Cout,Kpad], bias [Cout])."""
    import torch
    co, ci, ks, _ = w.shape
    return _pack("capf_op_pack_conv", w, bn, eps, (co, (ks * ks * ci + 31) // 32 * 32), torch.float32, co, ci, ks)


def conv_nhwc(x, wp, bias, ks, stride=1, act=0, residual=None):
    """x [B,H,W,Cin] cuda fp32 NHWC -> [B,Ho,Wo,Cout]."""
    d = ConvDesc()
    y = _conv_out(d, x, wp, bias, residual, wp.shape[0], ks, stride, act)
    _call("capf_op_conv", _stream(x), d.x, d.w_packed, d.bias, d.residual, d.y, d.B, d.H, d.W, d.Cin, d.Cout, ks, stride, act)
    return y


def pack_conv_wino(w, bn=None, eps=1e-5, variant=23):
    """w [Cout,Cin,3,3] cuda fp32 -> (Winograd weights [Cout, 12*Cin] for F(2,3) / [Cout, 18*Cin] for F(4,3), bias [Cout])."""
    import torch
    co, ci, ks, _ = w.shape
    assert ks == 3
    return _pack("capf_op_pack_conv_wino", w, bn, eps, (co, (18 if variant == 43 else 12) * ci), torch.float32, co, ci, variant)


def _wino_variant(wp, ci):
    return 43 if wp.shape[1] == 18 * ci else 23


def conv_nhwc_wino(x, wp, bias, act=0, residual=None):
    """3x3 stride-1 conv through the Winograd kernel (variant from the packed pitch): x [B,H,W,Cin] cuda fp32 NHWC -> [B,H,W,Cout]."""
    d = ConvDesc()
    y = _conv_out(d, x, wp, bias, residual, wp.shape[0], act=act)
    _call("capf_op_conv_wino", _stream(x), d.x, d.w_packed, d.bias, d.residual, d.y, d.B, d.H, d.W, d.Cin, d.Cout, act,
          _wino_variant(wp, d.Cin))
    return y


def conv_nhwc_wino_group(problems):
    """problems: list of (x, wp_wino, bias, act, residual) -> outputs; ONE grouped Winograd launch."""
    descs, outs = _conv_descs([(x, wp, bias, res, wp.shape[0], 3, 1, act) for x, wp, bias, act, res in problems])
    x0, wp0 = problems[0][:2]
    _call("capf_op_conv_wino_group", _stream(x0), len(problems), descs, _wino_variant(wp0, x0.shape[3]))
    return outs


def conv_nhwc_group(problems):
    """problems: list of (x, wp, bias, ks, stride, act, residual) -> list of outputs; ONE grouped launch."""
    descs, outs = _conv_descs([(x, wp, bias, res, wp.shape[0], ks, stride, act) for x, wp, bias, ks, stride, act, res in problems])
    _call("capf_op_conv_group", _stream(problems[0][0]), len(problems), descs)
    return outs


def pack_conv_bf16(w, bn=None, eps=1e-5):
    """-> (bf16 packed weights [Cout, Kpad64], fp32 bias [Cout])."""
    import torch
    co, ci, ks, _ = w.shape
    return _pack("capf_op_pack_conv_bf16", w, bn, eps, (co, (ks * ks * ci + 63) // 64 * 64), torch.bfloat16, co, ci, ks)


def conv_nhwc_bf16(x, wp, bias, ks, stride=1, act=0, residual=None):
    """x [B,H,W,Cin] cuda bf16 NHWC -> [B,Ho,Wo,Cout] bf16."""
    d = ConvDesc()
    y = _conv_out(d, x, wp, bias, residual, wp.shape[0], ks, stride, act, bf16=True)
    _call("capf_op_conv_bf16", _stream(x), d.x, d.w_packed, d.bias, d.residual, d.y, d.B, d.H, d.W, d.Cin, d.Cout, ks, stride, act)
    return y


def pack_conv_bf16_rh(w, bn=None, eps=1e-5):
    """3x3 weights for the row-halo bf16 conv -> (bf16 [Cout, 9 * Cin] in (kh, Cin / cw, kw, cw) order, fp32 bias, cw)."""
    import torch
    co, ci, ks, _ = w.shape
    cw = load_library().capf_op_conv_bf16_rh_width(ci)
    if ks != 3 or not cw:
        raise CapfError(f"row-halo conv needs a 3x3 kernel and Cin % 32 == 0 (got ks={ks}, Cin={ci})")
    return _pack("capf_op_pack_conv_bf16_rh", w, bn, eps, (co, 9 * ci), torch.bfloat16, co, ci) + (cw,)


def conv_nhwc_bf16_rh(x, wp, bias, act=0, residual=None):
    """x [B,H,W,Cin] cuda bf16 NHWC -> [B,H,W,Cout] bf16 (3x3, stride 1, pad 1)."""
    d = ConvDesc()
    y = _conv_out(d, x, wp, bias, residual, wp.shape[0], act=act, bf16=True)
    _call("capf_op_conv_bf16_rh", _stream(x), d.x, d.w_packed, d.bias, d.residual, d.y, d.B, d.H, d.W, d.Cin, d.Cout, act)
    return y


def pack_conv_bf16_ws(w, bn=None, eps=1e-5):
    """3x3 weights for the 2-D halo bf16 conv tile (csrc/igemm_bf16_ws.hip) -> (packed bf16 [elems], fp32 bias [Cout])."""
    import torch
    co, ci, ks, _ = w.shape
    n = load_library().capf_op_conv_bf16_ws_pack_elems(co, ci)
    if ks != 3 or n <= 0 or co % 8:
        raise CapfError(f"2-D halo conv needs a 3x3 kernel, Cin % 16 == 0 and Cout % 8 == 0 (got ks={ks}, Cin={ci}, Cout={co})")
    return _pack("capf_op_pack_conv_bf16_ws", w, bn, eps, n, torch.bfloat16, co, ci)


def conv_nhwc_bf16_ws_group(problems):
    """problems: list of (x, wp_ws, bias, act, residual, Cout), x / residual bf16 NHWC -> list of outputs (one grouped launch of the
    2-D halo tile, 3x3 / stride 1 / pad 1)."""
    descs, outs = _conv_descs([(x, wp, bias, res, co, 3, 1, act) for x, wp, bias, act, res, co in problems], bf16=True)
    _call("capf_op_conv_bf16_ws_group", _stream(problems[0][0]), len(problems), descs)
    return outs


def pack_conv_f32x3(w, bn=None, eps=1e-5):
    """3x3 weights for the split-fp32 conv tile (csrc/igemm_f32x3_ws.hip) -> (three bf16 pieces per weight, packed [elems]; fp32 bias [Cout])."""
    import torch
    co, ci, ks, _ = w.shape
    n = load_library().capf_op_conv_f32x3_pack_elems(co, ci)
    if ks != 3 or n <= 0 or co % 4:
        raise CapfError(f"split-fp32 conv needs a 3x3 kernel, Cin % 16 == 0 and Cout % 4 == 0 (got ks={ks}, Cin={ci}, Cout={co})")
    return _pack("capf_op_pack_conv_f32x3", w, bn, eps, n, torch.bfloat16, co, ci)


def conv_nhwc_f32x3_group(problems):
    """problems: list of (x, wp_x3, bias, act, residual, Cout), x / residual fp32 NHWC -> list of fp32 outputs (one grouped launch of the
    split-fp32 tile, 3x3 / stride 1 / pad 1)."""
    descs, outs = _conv_descs([(x, wp, bias, res, co, 3, 1, act) for x, wp, bias, act, res, co in problems])
    _call("capf_op_conv_f32x3_group", _stream(problems[0][0]), len(problems), descs)
    return outs


def pack_conv_f32h2(w, bn=None, eps=1e-5):
    """3x3 weights for the default split-fp32 conv tile (csrc/igemm_f32h2_ws.hip) -> (packed [elems] int16: two fp16 pieces per weight under
    one power-of-two scale per output channel, then the fp32 inverse scales; fp32 bias [Cout])."""
    import torch
    co, ci, ks, _ = w.shape
    n = load_library().capf_op_conv_f32h2_pack_elems(co, ci)
    if ks != 3 or n <= 0 or co % 4:
        raise CapfError(f"split-fp32 conv needs a 3x3 kernel, Cin % 16 == 0 and Cout % 4 == 0 (got ks={ks}, Cin={ci}, Cout={co})")
    return _pack("capf_op_pack_conv_f32h2", w, bn, eps, n, torch.int16, co, ci)


def conv_nhwc_f32h2_group(problems):
    """problems: list of (x, wp_h2, bias, act, residual, Cout), x / residual fp32 NHWC -> list of fp32 outputs (the level's launches of the
    two-fp16-piece tile, 3x3 / stride 1 / pad 1)."""
    descs, outs = _conv_descs([(x, wp, bias, res, co, 3, 1, act) for x, wp, bias, act, res, co in problems])
    _call("capf_op_conv_f32h2_group", _stream(problems[0][0]), len(problems), descs)
    return outs


def conv_nhwc_f32h2_planes(x, wp, bias, act, residual, cout, exps_in=None, planes_out=False):
    """One 3x3 / stride-1 conv on the two-fp16-piece tile with a PLANES tensor on one side (capf_op_conv_f32h2_planes): exps_in = the int32
    [tiles, Cin / 16] table of x's planes (x: the float32-typed tensor a planes_out conv returned); planes_out: y comes back as
    (float32-typed planes tensor, exps).  Use planes_to_fp32 to look at one."""
    import torch
    d = ConvDesc()
    y = _conv_out(d, x, wp, bias, residual, cout, act=act)
    tiles = load_library().capf_op_conv_f32h2_tiles(d.B, d.H, d.W, None)
    eo = torch.zeros(tiles, cout // 16, device=x.device, dtype=torch.int32) if planes_out else None
    _call("capf_op_conv_f32h2_planes", _stream(x), byref(d), _p(exps_in), _p(eo))
    return (y, eo) if planes_out else y


def f32h2_tile_pixels(B, H, W):
    """output pixels per tile of the two-fp16-piece conv tile at this geometry (flat pixel p belongs to tile p // that)"""
    px = c_int(0)
    if load_library().capf_op_conv_f32h2_tiles(B, H, W, byref(px)) <= 0:
        raise CapfError("geometry not eligible for the two-fp16-piece tile")
    return px.value


def planes_to_fp32(planes, exps, tile_pixels):
    """Decode a planes tensor [B, H, W, C] (float32-typed storage of [piece 0: 16 fp16 | piece 1: 16 fp16] per 16-channel chunk) with its
    [tiles, C / 16] exponent table into the fp32 values it stands for; tile_pixels: output pixels per tile (flat pixel p belongs to tile p // tile_pixels)."""
    import torch
    B, H, W, C = planes.shape
    h = planes.contiguous().view(torch.float16).view(B * H * W, C // 16, 2, 16).float()
    tile = torch.arange(B * H * W, device=planes.device) // tile_pixels
    scale = torch.exp2((127 - exps[tile].to(torch.float64))).to(torch.float32)                 # [pixels, C / 16]: 1 / 2^(se - 127)
    v = (h[:, :, 0, :] + h[:, :, 1, :]) * scale[:, :, None]
    return v.reshape(B, H, W, C)


def pack_f32h2_gemm(w, bn=None, eps=1e-5):
    """Weights for the two-fp16-piece GEMM (csrc/igemm_f32h2.hip): a conv filter [Cout, Cin, ks, ks] (BatchNorm folded if given) or an
    nn.Linear weight [N, K] -> (packed fp32-typed buffer [elems]: [N][Kpad] of {piece 0 | piece 1} chunks + [N] inverse scales; fp32 bias
    [N] for convs, None for linears)."""
    import torch
    if w.dim() == 4:
        n, ci, ks, _ = w.shape
        k = ks * ks * ci
    else:
        (n, k), ci, ks = w.shape, 0, 0
    elems = load_library().capf_op_f32h2_gemm_pack_elems(n, k)
    return _pack("capf_op_pack_f32h2_gemm", w, bn, eps, elems, torch.float32, n, ci, ks, k, bias="zeros" if w.dim() == 4 else None)


def conv_nhwc_f32h2g(x, wp, bias, ks, stride=1, act=0, residual=None, cout=None):
    """y = act(conv2d(x; two-fp16-piece pack) + bias (+ residual)), NHWC fp32, padding ks // 2, one launch of igemm_f32h2g."""
    d = ConvDesc()
    y = _conv_out(d, x, wp, bias, residual, cout if cout is not None else bias.numel(), ks, stride, act)
    _call("capf_op_conv_f32h2g", _stream(x), d.x, d.w_packed, d.bias, d.residual, d.y, d.B, d.H, d.W, d.Cin, d.Cout, ks, stride, act)
    return y


def conv_nhwc_f32h2g_group(problems):
    """problems: list of (x, wp, bias, ks, stride, act, residual, Cout) -> list of outputs, ONE grid of igemm_f32h2g_group_kernel."""
    descs, outs = _conv_descs([(x, wp, bias, res, co, ks, stride, act) for x, wp, bias, ks, stride, act, res, co in problems])
    _call("capf_op_conv_f32h2g_group", _stream(problems[0][0]), len(problems), descs)
    return outs


def _rows_out(x, n, dtype=None):
    import torch
    return torch.empty(x.shape[0], n, device=x.device, dtype=dtype or torch.float32)


def linear_ln_f32h2g(x, gamma, beta, eps, wp, bias, n, act=0, residual=None):
    """y[M, N] = act(LayerNorm(x[M, K]; gamma, beta, eps) @ W^T + bias (+ residual)) on the two-fp16-piece GEMM (K % 32 == 0, K <= 256, N % 4 == 0)."""
    (M, K), y = x.shape, _rows_out(x, n)
    _call("capf_op_linear_ln_f32h2g", _stream(x), _p(x), _p(gamma), _p(beta), float(eps), _p(wp), _p(bias), _p(residual), _p(y), M, n, K, act)
    return y


def linear_f32h2g(x, wp, bias, n, act=0, residual=None):
    """y[M, N] = act(x[M, K] @ W^T + bias (+ residual)) on the two-fp16-piece GEMM (K % 32 == 0, N % 4 == 0)."""
    (M, K), y = x.shape, _rows_out(x, n)
    _call("capf_op_linear_f32h2g", _stream(x), _p(x), _p(wp), _p(bias), _p(residual), _p(y), M, n, K, act)
    return y


def wgrad(dy, x, two_piece=True):
    """(dW[N, K], db[N]) = (dy[M, N]^T @ x[M, K], column sums of dy) through the training step's weight-gradient kernels."""
    import torch
    (M, N), K = dy.shape, x.shape[1]
    out = torch.empty(N * K + N, device=x.device, dtype=torch.float32)
    _call("capf_op_wgrad", _stream(x), _p(dy), _p(x), M, N, K, _p(out), 1 if two_piece else 0)
    return out[:N * K].view(N, K), out[N * K:]


def conv_nhwc_bf16_group(problems):
    """problems: list of (x, wp, bias, ks, stride, act, residual, wp_row_halo or None), all bf16 NHWC -> (outputs, variant)."""
    descs, outs = _conv_descs([(x, wp, bias, res, wp.shape[0], ks, stride, act) for x, wp, bias, ks, stride, act, res, _ in problems], bf16=True)
    rh = (c_void_p * len(problems))(*(p[7].data_ptr() if p[7] is not None else None for p in problems))
    variant = c_int32(-1)
    _call("capf_op_conv_bf16_group", _stream(problems[0][0]), len(problems), descs, rh, byref(variant))
    return outs, variant.value


# ---- the 16-bit kernel families for either element format: dtype = BF16 (the *_bf16 functions above, bit for bit) or F16 ----------
def pack_conv_16(w, bn=None, eps=1e-5, layout=0, dtype=F16):
    """BatchNorm fold + pack of w [Cout,Cin,k,k] in the 16-bit format `dtype`; layout 0: [Cout, Kpad64] (pack_conv_bf16), 1: row-halo
    [Cout, 9 * Cin] (pack_conv_bf16_rh), 2: the 2-D halo tile's [elems] (pack_conv_bf16_ws) -> (packed weights, fp32 bias [Cout])."""
    co, ci, ks, _ = w.shape
    if layout == 0:
        shape = (co, (ks * ks * ci + 63) // 64 * 64)
    elif layout == 1:
        shape = (co, 9 * ci)
    else:
        shape = load_library().capf_op_conv_bf16_ws_pack_elems(co, ci)
        if shape <= 0:
            raise CapfError(f"2-D halo conv needs Cin % 16 == 0 (got Cin={ci})")
    return _pack("capf_op_pack_conv_16", w, bn, eps, shape, _TORCH16_OF[dtype](), co, ci, ks, layout, dtype)


def conv_nhwc_16(x, wp, bias, ks, stride=1, act=0, residual=None, dtype=F16):
    """x [B,H,W,Cin] cuda NHWC in the 16-bit format `dtype` -> [B,Ho,Wo,Cout] in the same (conv_nhwc_bf16).  Cin % 8 != 0: the stem of a
    16-bit plan -- x is the fp32 image, wp / bias the fp32 pack of pack_conv, no residual; the result is 16-bit."""
    d = ConvDesc()
    y = _conv_out(d, x, wp, bias, residual, wp.shape[0], ks, stride, act, dtype=_TORCH16_OF[dtype]())
    _call("capf_op_conv_16", _stream(x), d.x, d.w_packed, d.bias, d.residual, d.y, d.B, d.H, d.W, d.Cin, d.Cout, ks, stride, act, dtype)
    return y


def conv_nhwc_16_group(problems, dtype=F16):
    """conv_nhwc_bf16_group for either format: (x, wp, bias, ks, stride, act, residual, wp_row_halo or None) each -> (outputs, variant)."""
    descs, outs = _conv_descs([(x, wp, bias, res, wp.shape[0], ks, stride, act) for x, wp, bias, ks, stride, act, res, _ in problems],
                              dtype=_TORCH16_OF[dtype]())
    rh = (c_void_p * len(problems))(*[(p[7].data_ptr() if p[7] is not None else None) for p in problems])
    variant = c_int32(-1)
    _call("capf_op_conv_16_group", _stream(problems[0][0]), len(problems), descs, rh, byref(variant), dtype)
    return outs, variant.value


def conv_nhwc_16_ws_group(problems, dtype=F16):
    """conv_nhwc_bf16_ws_group for either format: (x, wp_ws, bias, act, residual, Cout) each -> outputs (one launch of the 2-D halo tile)."""
    descs, outs = _conv_descs([(x, wp, bias, res, co, 3, 1, act) for x, wp, bias, act, res, co in problems], dtype=_TORCH16_OF[dtype]())
    _call("capf_op_conv_16_ws_group", _stream(problems[0][0]), len(problems), descs, dtype)
    return outs


def linear_16(x, w, bias=None, residual=None, gelu=False, dtype=F16):
    """linear_bf16 for either format: x [M,K], w [N,K] 16-bit -> fp32 [M,N] (+ fp32 residual), or gelu=True -> 16-bit GELU(x w^T + b)."""
    M, K = x.shape
    N = w.shape[0]
    y = _rows_out(x, N, _TORCH16_OF[dtype]() if gelu else None)
    _call("capf_op_linear_16", _stream(x), _p(x.contiguous()), _p(w.contiguous()), _p(bias), _p(residual), _p(y), M, N, K, 1 if gelu else 0, dtype)
    return y


def bneck_16(x, packs, tap=False, dtype=F16):
    """A layer1 bottleneck as ONE kernel (csrc/bneck_bf16.hip).  x [B,H,W,64] with packs = [(wp, bias)] * 4 for conv1, conv2, conv3 and the
    downsample conv (the first bottleneck), or x [B,H,W,256] with three packs (an identity bottleneck); weights from pack_conv_16 layout 0.
    -> (y [B,H,W,256], t1, t2, shortcut or None): t1 / t2 / shortcut hold conv1's, conv2's and the downsample's outputs only with tap."""
    import torch
    B, H, W, _ = x.shape
    first = len(packs) == 4
    new = lambda c: torch.empty(B, H, W, c, device=x.device, dtype=x.dtype)
    t1, t2, y, sc = new(64), new(64), new(256), (new(256) if first else None)
    w = (c_void_p * 4)(*[packs[i][0].data_ptr() if i < len(packs) else None for i in range(4)])
    b = (c_void_p * 4)(*[packs[i][1].data_ptr() if i < len(packs) else None for i in range(4)])
    _call("capf_op_bneck_16", _stream(x), _p(x), w, b, _p(t1), _p(t2), _p(sc), _p(y), B, H, W, 1 if tap else 0, dtype)
    return y, t1, t2, sc


def f16_round_host(values):
    """The library's float -> fp16 store rule on the host (capf_debug_f16_round): fp32 numpy array -> uint16 bit patterns."""
    import numpy as np
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    out = np.empty(v.size, dtype=np.uint16)
    _call("capf_debug_f16_round", v.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p), int(v.size))
    return out.reshape(np.shape(values))


def linear(x, w, bias=None, act=0, residual=None):
    (M, K), y = x.shape, _rows_out(x, w.shape[0])
    _call("capf_op_linear", _stream(x), _p(x), _p(w), _p(bias), _p(residual), _p(y), M, w.shape[0], K, act)
    return y


def bilinear_corners(grid, H, W, border):
    """grid: CUDA fp32 [..., 2] normalised (x, y) -> (idx int32 [..., 2] = NW corner (x0, y0), frac fp32 [..., 2]) by the
    device function both sampling sites of capf_forward use."""
    import torch
    g = grid.contiguous()
    idx = torch.empty(g.shape, dtype=torch.int32, device=g.device)
    frac = torch.empty(g.shape, dtype=torch.float32, device=g.device)
    _call("capf_op_bilinear_corners", _stream(g), _p(g), g.numel() // 2, int(H), int(W), 1 if border else 0, _p(idx), _p(frac))
    return idx, frac


def bn_stats(x, gamma, beta, eps=1e-5, momentum=0.1, running_mean=None, running_var=None):
    """Batch statistics of x [rows, C] (fp32, contiguous) as capf_backbone_forward_bn takes them (capf_op_bn_stats): returns
    (scale, shift) with scale = gamma / sqrt(var + eps), shift = beta - mean * scale; running_mean / running_var are updated in place."""
    import torch
    rows, C = x.shape
    nbytes = load_library().capf_op_bn_stats_scratch_bytes(rows, C)
    scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=x.device)
    scale = torch.empty(C, dtype=torch.float32, device=x.device)
    shift = torch.empty(C, dtype=torch.float32, device=x.device)
    _call("capf_op_bn_stats", _stream(x), _p(x), rows, C, _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean), _p(running_var),
          _p(scale), _p(shift), _p(scratch), nbytes)
    return scale, shift


def bn_apply(x, scale, shift, residual=None, relu=False, out=None):
    """y = act(x * scale[c] + shift[c] + residual) on x [rows, C] (capf_op_bn_apply); out may be x (in place)."""
    import torch
    rows, C = x.shape
    y = torch.empty_like(x) if out is None else out
    _call("capf_op_bn_apply", _stream(x), _p(x), _p(scale), _p(shift), _p(residual), _p(y), rows, C, 1 if relu else 0)
    return y


KP_ARGMAX, KP_INTEGRAL = 0, 1     # capf_kp_head_forward's `mode`
KP_MODES = {"argmax": KP_ARGMAX, "integral": KP_INTEGRAL}


def _kp_map_dtype(x):
    """capf_dtype of a map tensor (fp32 / bf16 / fp16); anything else is refused here, not converted"""
    import torch
    code = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}.get(x.dtype)
    if code is None or x.dim() != 4 or not x.is_contiguous():
        raise CapfError(f"the keypoint head takes a contiguous NHWC map [B, H, W, C] of fp32 / bf16 / fp16, not {tuple(x.shape)} {x.dtype}")
    return code


def _kp_weight(weight, C):
    """the 1x1 conv weight [J, C] or [J, C, 1, 1] as (contiguous fp32 [J, C], J)"""
    import torch
    w = weight.reshape(weight.shape[0], -1)
    if w.shape[1] != C or w.dtype != torch.float32 or not w.is_contiguous():
        raise CapfError(f"the keypoint head's weight must be contiguous fp32 [J, {C}] (or [J, {C}, 1, 1]), not {tuple(weight.shape)} {weight.dtype}")
    return w, w.shape[0]


def _kp_to_image(to_image, B):
    import torch
    if to_image is not None and (tuple(to_image.shape) != (B, 2, 3) or to_image.dtype != torch.float32 or not to_image.is_contiguous()):
        raise CapfError(f"to_image must be contiguous fp32 [{B}, 2, 3], not {tuple(to_image.shape)} {to_image.dtype}")


def _kp_pair_split(x2):
    """(Bsrc, H, W, C) of a flip-test pair's map [2 * Bsrc, H, W, C]"""
    if x2.shape[0] % 2:
        raise CapfError(f"a flip-test pair holds 2 * Bsrc frames ([orig | mirrored]), not {x2.shape[0]}")
    return x2.shape[0] // 2, x2.shape[1], x2.shape[2], x2.shape[3]


def _kp_swap(swap, J, what):
    """a pair entry's `swap` as the C array of J ints: None is H36M_SWAP, at 17 joints only; `what`: "a head of" / "a decode of" """
    if swap is None:
        if J != 17:
            raise CapfError(f"swap=None means the H36M table (17 joints); {what} {J} joints needs its own table")
        swap = H36M_SWAP
    tab = [int(v) for v in swap]
    if len(tab) != J:
        raise CapfError(f"swap has {len(tab)} entries for {J} joints")
    return (c_int32 * max(J, 1))(*tab)


def _kp_outputs(x, lead, J, to_image, want_score):
    """fresh fp32 (kcrop, k2d | None, score | None) beside the map x: lead = (B,), or (2, Bsrc) for a pair's stacks"""
    import torch
    f32, dev = torch.float32, x.device
    return (torch.empty(*lead, J, 2, dtype=f32, device=dev), torch.empty(*lead, J, 2, dtype=f32, device=dev) if to_image is not None else None,
            torch.empty(lead[-1], J, dtype=f32, device=dev) if want_score else None)


def _kp_decode(decode):
    return (c_float * 4)(*[float(v) for v in decode])


def _kp_common(x, weight, decode, to_image, backward):
    import torch
    B, H, W, C = x.shape
    w, J = _kp_weight(weight, C)
    _kp_to_image(to_image, B)
    nbytes = load_library().capf_kp_head_scratch_bytes(B, H, W, C, J, 1 if backward else 0)
    return (B, H, W, C, J), w, _kp_decode(decode), torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device), nbytes


def kp_head_forward(x, weight, bias=None, mode=KP_ARGMAX, beta=1.0, decode=(1.0, 0.0, 1.0, 0.0), to_image=None, want_score=True,
                    want_heat=False):
    """capf_kp_head_forward on a contiguous NHWC map x [B, H, W, C] (fp32 / bf16 / fp16): the 1x1 conv weight [J, C] (+ bias [J]) and the
    heatmap decode (mode KP_ARGMAX / KP_INTEGRAL with `beta`) in one pass.  decode = (sx, ox, sy, oy) maps heatmap to crop coordinates;
    to_image [B, 2, 3] fp32 (crop_to_image_matrix) maps those to the lifter's normalised image coordinates.
    Returns (kcrop [B, J, 2], score [B, J] | None, k2d [B, J, 2] | None, heat [B, J, H, W] | None)."""
    import torch
    dtype = _kp_map_dtype(x)
    (B, H, W, C, J), w, dec, scratch, nbytes = _kp_common(x, weight, decode, to_image, False)
    kcrop, k2d, score = _kp_outputs(x, (B,), J, to_image, want_score)
    heat = torch.empty(B, J, H, W, dtype=torch.float32, device=x.device) if want_heat else None
    _call("capf_kp_head_forward", _stream(x), _p(x), dtype, _p(w), _p(bias), B, H, W, C, J, int(mode), float(beta), dec, _p(to_image),
          _p(kcrop), _p(k2d), _p(score), _p(heat), _p(scratch), nbytes)
    return kcrop, score, k2d, heat


def kp_head_backward(x, weight, bias=None, dkcrop=None, dk2d=None, beta=1.0, decode=(1.0, 0.0, 1.0, 0.0), to_image=None, want_dmap=False,
                     dmap=None):
    """capf_kp_head_backward (integral decode, fp32 map): gradients of sum(dkcrop * kcrop) + sum(dk2d * k2d).  Returns (dweight [J, C],
    dbias [J] -- exact zeros --, dmap | None).  dmap given: the map gradient is ADDED to it (capf_backward_points' dfeat_nhwc[0]);
    want_dmap without dmap: a fresh tensor, overwritten."""
    import torch
    dtype = _kp_map_dtype(x)
    (B, H, W, C, J), w, dec, scratch, nbytes = _kp_common(x, weight, decode, to_image, True)
    for name, g in (("dkcrop", dkcrop), ("dk2d", dk2d)):
        if g is not None and (tuple(g.shape) != (B, J, 2) or g.dtype != torch.float32 or not g.is_contiguous()):
            raise CapfError(f"{name} must be contiguous fp32 [{B}, {J}, 2], not {tuple(g.shape)} {g.dtype}")
    accumulate = dmap is not None
    if accumulate and (dmap.shape != x.shape or dmap.dtype != torch.float32 or not dmap.is_contiguous()):
        raise CapfError(f"dmap must be contiguous fp32 {tuple(x.shape)}, not {tuple(dmap.shape)} {dmap.dtype}")
    if dmap is None and want_dmap:
        dmap = torch.empty(B, H, W, C, dtype=torch.float32, device=x.device)
    dw = torch.empty(J, C, dtype=torch.float32, device=x.device)
    db = torch.empty(J, dtype=torch.float32, device=x.device)
    _call("capf_kp_head_backward", _stream(x), _p(dkcrop), _p(dk2d), _p(x), dtype, _p(w), _p(bias), B, H, W, C, J, KP_INTEGRAL, float(beta),
          dec, _p(to_image), _p(dw), _p(db), _p(dmap), 1 if accumulate else 0, _p(scratch), nbytes)
    return dw, db, dmap


KP_LOSS_MEAN, KP_LOSS_OHKM = 0, 1     # capf_kp_heatmap_loss's `reduction`
KP_LOSS_REDUCTIONS = {"mean": KP_LOSS_MEAN, "ohkm": KP_LOSS_OHKM}


def kp_heatmap_loss(x, weight, bias=None, kcrop_gt=None, target_weight=None, decode=(1.0, 0.0, 1.0, 0.0), sigma=2.0, reduction="mean", topk=8,
                    scale=0.5, want_grads=True, want_dmap=False, dmap_accumulate_into=None):
    """capf_kp_heatmap_loss on a contiguous NHWC map x [B, H, W, C] (fp32 / bf16 / fp16): the 1x1 conv weight [J, C] (+ bias [J]), the Gaussian
    targets around kcrop_gt [B, J, 2] (crop pixels; decode = (sx, ox, sy, oy) maps heatmap to crop coordinates), the weighted mean-squared
    error (reduction "mean" / "ohkm" with `topk`, or KP_LOSS_MEAN / KP_LOSS_OHKM) and its gradients in one native call.
    Returns (loss [1], joint_loss [B, J], dweight [J, C] | None, dbias [J] | None, dmap | None).  dmap_accumulate_into given: the map gradient
    is ADDED to it (capf_backward_points' dfeat_nhwc[0]); want_dmap without it: a fresh tensor, overwritten.  The map gradient needs an fp32 map."""
    import torch
    if isinstance(reduction, str):
        if reduction not in KP_LOSS_REDUCTIONS:
            raise ValueError(f"reduction must be 'mean' or 'ohkm', got {reduction!r}")
        reduction = KP_LOSS_REDUCTIONS[reduction]
    dtype = _kp_map_dtype(x)
    B, H, W, C = x.shape
    w, J = _kp_weight(weight, C)
    f32, dev = torch.float32, x.device
    if kcrop_gt is None or tuple(kcrop_gt.shape) != (B, J, 2) or kcrop_gt.dtype != f32 or not kcrop_gt.is_contiguous():
        raise CapfError(f"kcrop_gt must be contiguous fp32 [{B}, {J}, 2], not {None if kcrop_gt is None else (tuple(kcrop_gt.shape), kcrop_gt.dtype)}")
    if target_weight is not None:
        target_weight = target_weight.reshape(B, J) if target_weight.numel() == B * J else target_weight
        if tuple(target_weight.shape) != (B, J) or target_weight.dtype != f32 or not target_weight.is_contiguous():
            raise CapfError(f"target_weight must be contiguous fp32 [{B}, {J}] (or [{B}, {J}, 1]), not {tuple(target_weight.shape)} {target_weight.dtype}")
    dmap = dmap_accumulate_into
    accumulate = dmap is not None
    if accumulate and (dmap.shape != x.shape or dmap.dtype != f32 or not dmap.is_contiguous()):
        raise CapfError(f"dmap_accumulate_into must be contiguous fp32 {tuple(x.shape)}, not {tuple(dmap.shape)} {dmap.dtype}")
    if dmap is None and want_dmap:
        dmap = torch.empty(B, H, W, C, dtype=f32, device=dev)
    nbytes = load_library().capf_kp_heatmap_loss_scratch_bytes(B, H, W, C, J, int(reduction))
    scratch = torch.empty(max(nbytes, 4) // 4, dtype=f32, device=dev)
    loss = torch.empty(1, dtype=f32, device=dev)
    joint_loss = torch.empty(B, J, dtype=f32, device=dev)
    dw = torch.empty(J, C, dtype=f32, device=dev) if want_grads else None
    db = torch.empty(J, dtype=f32, device=dev) if want_grads else None
    _call("capf_kp_heatmap_loss", _stream(x), _p(x), dtype, _p(w), _p(bias), B, H, W, C, J, _p(kcrop_gt), _p(target_weight), _kp_decode(decode),
          float(sigma), int(reduction), int(topk), float(scale), _p(loss), _p(joint_loss), _p(dw), _p(db), _p(dmap), 1 if accumulate else 0,
          _p(scratch), nbytes)
    return loss, joint_loss, dw, db, dmap


def cpn_decode_taps():
    """capf_cpn_decode_taps: the 21 Gaussian taps of capf_cpn_decode's blur as Python floats (host code, no GPU needed)"""
    g = (c_double * 21)()
    load_library().capf_cpn_decode_taps(g)
    return list(g)


def cpn_decode(heat, joints=None, decode=(1.0, 0.0, 1.0, 0.0), to_image=None, want_score=True, want_blurred=False):
    """capf_cpn_decode on a contiguous NHWC heatmap tensor heat [B, H, W, C] (fp32 / bf16 / fp16; Engine.tensor_view("heat", B) of a
    PLAN_CPN_PREDICT handle): CPN's two-peak decode of channels 0 .. joints - 1 (default: all C).  decode = (sx, ox, sy, oy) maps heatmap
    to crop coordinates (CPN: sx = W_img / W, ox = sx / 2, the same in y); to_image [B, 2, 3] fp32 (crop_to_image_matrix) maps those to the
    lifter's normalised image coordinates.
    Returns (kcrop [B, J, 2], score [B, J] | None, k2d [B, J, 2] | None, blurred [B, J, H + 20, W + 20] float64 | None)."""
    import torch
    dtype = _kp_map_dtype(heat)
    B, H, W, C = heat.shape
    J = C if joints is None else int(joints)
    _kp_to_image(to_image, B)
    kcrop, k2d, score = _kp_outputs(heat, (B,), J, to_image, want_score)
    blurred = torch.empty(B, J, H + 20, W + 20, dtype=torch.float64, device=heat.device) if want_blurred else None
    _call("capf_cpn_decode", _stream(heat), _p(heat), dtype, B, H, W, C, J, _kp_decode(decode), _p(to_image), _p(kcrop), _p(k2d), _p(score),
          _p(blurred))
    return kcrop, score, k2d, blurred


# the H36M skeleton's mirror table: joints_left [4, 5, 6, 11, 12, 13] <-> joints_right [1, 2, 3, 14, 15, 16] (mvn/datasets/utils.py:12-13;
# kSwap of csrc/preprocess.hip, the table capf_fliptest_fuse and capf_preprocess_points apply)
H36M_SWAP = (0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13)
# the mirror table of a checkpoint whose 17 channels are in COCO order: nose | eyes | ears | shoulders | elbows | wrists | hips | knees | ankles
# (upstream CPN's cfg.symmetry).  The defaults stay H36M_SWAP: the keypoints of this module feed the H36M lifter.
COCO_SWAP = (0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15)


def cpn_decode_pair(heat2, joints=None, swap=None, decode=(1.0, 0.0, 1.0, 0.0), to_image=None, mirror_width=192.0, want_score=True,
                    want_blurred=False, want_fused=False):
    """capf_cpn_decode_pair on the contiguous NHWC heatmaps heat2 [2 * Bsrc, H, W, C] of a flip-test pair (frame Bsrc + b the mirror of frame b,
    the order of capf_preprocess mode 2; Engine.tensor_view("heat", 2 * Bsrc) of a PLAN_CPN_PREDICT handle): CPN's test-time flip -- per joint
    the heatmap of the crop and the mirrored-back heatmap of its mirror (x mirrored, joints exchanged by `swap`, no column shift) are averaged
    and decoded once with cpn_decode's rule.  joints: channels 0 .. joints - 1 (default: all C).  swap: J ints, swap[j] = the joint of the
    mirror that lands on joint j, its own inverse; None: H36M_SWAP (J = 17 only).  to_image [Bsrc, 2, 3].
    Returns (kcrop2 [2, Bsrc, J, 2], score [Bsrc, J] | None, k2d2 [2, Bsrc, J, 2] | None, blurred [Bsrc, J, H + 20, W + 20] float64 | None,
    fused [Bsrc, J, H, W] | None -- the averaged heatmaps): kcrop2 / k2d2 are the stacks forward_flip_test takes, set 1 mirrored like
    preprocess_points(mode=2) with `mirror_width` in place of its 192."""
    import torch
    dtype = _kp_map_dtype(heat2)
    Bsrc, H, W, C = _kp_pair_split(heat2)
    J = C if joints is None else int(joints)
    tab = _kp_swap(swap, J, "a decode of")
    _kp_to_image(to_image, Bsrc)
    kcrop2, k2d2, score = _kp_outputs(heat2, (2, Bsrc), J, to_image, want_score)
    blurred = torch.empty(Bsrc, J, H + 20, W + 20, dtype=torch.float64, device=heat2.device) if want_blurred else None
    fused = torch.empty(Bsrc, J, H, W, dtype=torch.float32, device=heat2.device) if want_fused else None
    _call("capf_cpn_decode_pair", _stream(heat2), _p(heat2), dtype, Bsrc, H, W, C, J, tab, _kp_decode(decode), _p(to_image), float(mirror_width),
          _p(kcrop2), _p(k2d2), _p(score), _p(blurred), _p(fused))
    return kcrop2, score, k2d2, blurred, fused


def kp_head_forward_pair(x2, weight, bias=None, mode=KP_ARGMAX, beta=1.0, swap=None, shift=True, decode=(1.0, 0.0, 1.0, 0.0), to_image=None,
                         mirror_width=192.0, want_score=True, want_heat=False):
    """capf_kp_head_forward_pair on the contiguous NHWC map x2 [2 * Bsrc, H, W, C] of a flip-test pair (frame Bsrc + b the mirror of frame b,
    the order of capf_preprocess mode 2): the heatmaps of each crop and of its flipped-back mirror are averaged (`shift`: HRNet's one-column
    SHIFT_HEATMAP) and decoded once.  swap: J ints, swap[j] = the joint of the mirror that lands on joint j, its own inverse; None: H36M_SWAP
    (J = 17 only).  to_image [Bsrc, 2, 3].  Returns (kcrop2 [2, Bsrc, J, 2], score [Bsrc, J] | None, k2d2 [2, Bsrc, J, 2] | None,
    heat [Bsrc, J, H, W] | None -- the fused logits): kcrop2 / k2d2 are the stacks forward_flip_test takes, set 1 mirrored like
    preprocess_points(mode=2) with `mirror_width` in place of its 192."""
    import torch
    dtype = _kp_map_dtype(x2)
    Bsrc, H, W, C = _kp_pair_split(x2)
    w, J = _kp_weight(weight, C)
    tab = _kp_swap(swap, J, "a head of")
    _kp_to_image(to_image, Bsrc)
    nbytes = load_library().capf_kp_head_pair_scratch_bytes(Bsrc, H, W, C, J)
    scratch = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x2.device)
    kcrop2, k2d2, score = _kp_outputs(x2, (2, Bsrc), J, to_image, want_score)
    heat = torch.empty(Bsrc, J, H, W, dtype=torch.float32, device=x2.device) if want_heat else None
    _call("capf_kp_head_forward_pair", _stream(x2), _p(x2), dtype, _p(w), _p(bias), Bsrc, H, W, C, J, int(mode), float(beta), tab,
          1 if shift else 0, _kp_decode(decode), _p(to_image), float(mirror_width), _p(kcrop2), _p(k2d2), _p(score), _p(heat), _p(scratch), nbytes)
    return kcrop2, score, k2d2, heat


def linear_bf16(x, w, bias=None, residual=None, gelu=False):
    """x bf16 [M,K], w bf16 [N,K] -> fp32 [M,N] (+ fp32 residual), or with gelu=True -> bf16 GELU(x w^T + b)."""
    import torch
    (M, K), N = x.shape, w.shape[0]
    y = _rows_out(x, N, torch.bfloat16 if gelu else torch.float32)
    _call("capf_op_linear_bf16", _stream(x), _p(x.contiguous()), _p(w.contiguous()), _p(bias), _p(residual), _p(y), M, N, K, 1 if gelu else 0)
    return y


# ---- neighbours of the path: N1 preprocessing, N2 flip-test fusion -------------------------------------
HRNET_MEAN, HRNET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # datasets/utils.py:24-26
CPN_MEAN = tuple(v / 255.0 for v in (122.7717, 115.9465, 102.9801))             # :27-29


def preprocess(images_u8, gt, k2d, kcrop, backbone="hrnet_32", mode=0):
    """uint8 BGR [B,H,W,3] + labels (all CUDA) -> (images fp32 RGB NHWC, gt root-relative, k2d, kcrop).
    mode 0 plain, 1 train-time horizontal flip, 2 flip-test ([2,B,...] outputs: original then mirrored)."""
    import torch
    lib = load_library()
    B, H, W, _ = images_u8.shape
    nsets = 2 if mode == 2 else 1
    dev = images_u8.device
    img_out = torch.empty((nsets, B, H, W, 3) if nsets == 2 else (B, H, W, 3), dtype=torch.float32, device=dev)
    k2d_out = torch.empty((nsets, B, 17, 2) if nsets == 2 else (B, 17, 2), dtype=torch.float32, device=dev)
    kc_out = torch.empty(k2d_out.shape, dtype=torch.float32, device=dev)
    gt_out = torch.empty(gt.shape, dtype=torch.float32, device=dev) if gt is not None else None
    if backbone == "cpn":
        mean = torch.tensor([122.7717, 115.9465, 102.9801]) / 255.0              # fp32 division, like the reference
        std = None
    else:
        mean, std = torch.tensor(HRNET_MEAN), torch.tensor(HRNET_STD)
    m3 = (c_float * 3)(*mean.tolist())
    s3 = (c_float * 3)(*std.tolist()) if std is not None else None
    rc = lib.capf_preprocess(_stream(images_u8), _p(images_u8.contiguous()), B, H, W, m3, s3, mode, _p(img_out),
                             _p(gt.contiguous()) if gt is not None else c_void_p(0), _p(gt_out), _p(k2d.contiguous()), _p(k2d_out),
                             _p(kcrop.contiguous()), _p(kc_out))
    if rc:
        raise CapfError(f"capf_preprocess failed ({rc})")
    return img_out, gt_out, k2d_out, kc_out


def input_constants(backbone="hrnet_32"):
    """(mean, std) of data_prefetcher for a backbone as (c_float * 3) arrays in RGB order; std None: mean only (cpn).  The values preprocess() uses."""
    import torch
    if backbone == "cpn":
        mean, std = torch.tensor([122.7717, 115.9465, 102.9801]) / 255.0, None       # fp32 division, like the reference
    else:
        mean, std = torch.tensor(HRNET_MEAN), torch.tensor(HRNET_STD)
    return (c_float * 3)(*mean.tolist()), ((c_float * 3)(*std.tolist()) if std is not None else None)


def preprocess_points(gt, k2d, kcrop, mode=0):
    """The points half of preprocess() alone (capf_preprocess_points): -> (gt root-relative or None, k2d, kcrop), [2,B,17,2] in mode 2."""
    import torch
    B = k2d.shape[0]
    shape = (2, B, 17, 2) if mode == 2 else (B, 17, 2)
    k2d_out = torch.empty(shape, dtype=torch.float32, device=k2d.device)
    kc_out = torch.empty_like(k2d_out)
    gt_out = torch.empty_like(gt) if gt is not None else None
    _call("capf_preprocess_points", _stream(k2d), B, int(mode), _p(gt.contiguous()) if gt is not None else c_void_p(0), _p(gt_out),
          _p(k2d.contiguous()), _p(k2d_out), _p(kcrop.contiguous()), _p(kc_out))
    return gt_out, k2d_out, kc_out


def input_rule_host(u, channel, mean, std=None):
    """The input normalisation rule on the host (capf_input_rule_host): uint8 numpy array, RGB channel index, mean / std sequences of 3
    floats (std None: mean only) -> fp32 numpy array of the same shape."""
    import numpy as np
    v = np.ascontiguousarray(u, dtype=np.uint8).reshape(-1)
    out = np.empty(v.size, dtype=np.float32)
    m3 = (c_float * 3)(*[float(x) for x in mean])
    s3 = (c_float * 3)(*[float(x) for x in std]) if std is not None else None
    _call("capf_input_rule_host", v.ctypes.data_as(c_void_p), int(v.size), int(channel), m3, s3, out.ctypes.data_as(c_void_p))
    return out.reshape(np.shape(u))


def op_conv_u8(images_u8, wp, bias, ks, stride=1, act=0, mode=0, mean=HRNET_MEAN, std=HRNET_STD, dtype=F32):
    """The stem conv from a uint8 BGR image [Bsrc,H,W,3] (CUDA, any alignment; a view at a byte offset of a larger buffer is fine as long as
    it is dense): wp / bias from pack_conv (Cin = 3) -> [frames,Ho,Wo,Cout] of `dtype` (F32 / BF16 / F16), frames = Bsrc or 2 * Bsrc (mode 2)."""
    import torch
    Bsrc, H, W, _ = images_u8.shape
    if images_u8.dtype != torch.uint8 or not images_u8.is_contiguous():
        raise CapfError("op_conv_u8 needs a dense uint8 [Bsrc,H,W,3] tensor")
    frames = Bsrc * (2 if mode == 2 else 1)
    y = torch.empty(frames, *_out_hw(H, W, ks, stride), wp.shape[0], device=images_u8.device,
                    dtype=torch.float32 if dtype == F32 else _TORCH16_OF[dtype]())
    m3 = (c_float * 3)(*[float(x) for x in mean])
    s3 = (c_float * 3)(*[float(x) for x in std]) if std is not None else None
    _call("capf_op_conv_u8", _stream(images_u8), _p(images_u8), _p(wp), _p(bias), _p(y), Bsrc, int(mode), H, W, wp.shape[0], ks, stride, act,
          m3, s3, dtype)
    return y


def op_conv_u8_kernel_name(Bsrc, mode, H, W, cout, ks, stride, dtype=F32):
    """The kernel op_conv_u8 launches for this problem; stem_kernel_name: the float stem op's (conv_nhwc / conv_nhwc_16 on an fp32 image)."""
    return load_library().capf_op_conv_u8_kernel_name(Bsrc, mode, H, W, cout, ks, stride, dtype).decode()


def stem_kernel_name(B, H, W, cout, ks, stride, dtype=F32):
    return load_library().capf_op_conv_stem_kernel_name(B, H, W, cout, ks, stride, dtype).decode()


# the 3DHP skeleton's mirror table: joints_left [5, 6, 7, 11, 12, 13] <-> joints_right [2, 3, 4, 8, 9, 10] (ContextPose_mpi/run_3dhp.py:45-46)
MPI_SWAP = (0, 1, 5, 6, 7, 2, 3, 4, 11, 12, 13, 8, 9, 10, 14, 15, 16)


def fliptest_fuse(pred2, swap=None):
    """pred2 [2,B,1,J,3] (original, mirrored) -> [B,1,J,3]: the mirrored prediction's x negated, its joints swapped, the mean of the
    two.  swap None: the H36M table of train.py:177-180 (capf_fliptest_fuse, J = 17); else a sequence of J ints, swap[j] = the joint of
    the mirrored prediction that lands on joint j (MPI_SWAP: run_3dhp.py:169-180), a permutation that is its own inverse."""
    import torch
    lib = load_library()
    B, J = pred2.shape[1], pred2.shape[-2]
    out = torch.empty(B, 1, J, 3, dtype=torch.float32, device=pred2.device)
    if swap is None:
        rc = lib.capf_fliptest_fuse(_stream(pred2), _p(pred2.contiguous()), B, _p(out))
    else:
        tab = [int(v) for v in swap]
        if len(tab) != J:
            raise ValueError(f"swap has {len(tab)} entries for {J} joints")
        rc = lib.capf_fliptest_fuse_swap(_stream(pred2), _p(pred2.contiguous()), B, J, (c_int32 * J)(*tab), _p(out))
    if rc:
        raise CapfError(f"capf_fliptest_fuse{'' if swap is None else '_swap'} failed ({rc})")
    return out


# ---- N3: affine crop (mvn/utils/img.py) ---------------------------------------------------------------
def affine_from_center_scale(center, scale, output_size):
    """get_affine_transform(center, scale, 0, output_size) -> 2x3 float64 numpy matrix (host code, no GPU)."""
    import numpy as np
    lib = load_library()
    c = (c_double * 2)(float(center[0]), float(center[1]))
    sc = (c_double * 2)(float(scale[0]), float(scale[1]))
    m = (c_double * 6)()
    rc = lib.capf_affine_from_center_scale(c, sc, int(output_size[0]), int(output_size[1]), m)
    if rc:
        raise CapfError(f"capf_affine_from_center_scale failed ({rc})")
    return np.array(list(m), dtype=np.float64).reshape(2, 3)


def crop_to_image_matrix(center, scale, output_size, res_w, res_h):
    """The 2x3 float64 matrix that takes crop pixel coordinates (x, y, 1) of the crop affine_from_center_scale(center, scale, output_size)
    cuts to the lifter's normalised image coordinates: the inverse of that affine followed by normalize_screen_coordinates
    (common/camera.py:14-18: X / w * 2 - [1, h / w]) for an image of res_w x res_h pixels.  Host code; one row of kp_head_forward's to_image."""
    import numpy as np
    m = np.vstack([affine_from_center_scale(center, scale, output_size), [0.0, 0.0, 1.0]])
    inv = np.linalg.inv(m)[:2]
    a = inv * (2.0 / float(res_w))
    a[0, 2] -= 1.0
    a[1, 2] -= float(res_h) / float(res_w)
    return a


def warp_affine(frames, mats, output_size):
    """frames: list of uint8 CUDA tensors [H_i, W_i, 3] (BGR as cv2.imread gives them); mats: [B, 2, 3] float64
    forward matrices (numpy or tensor); output_size = (out_w, out_h) -> uint8 CUDA tensor [B, out_h, out_w, 3]."""
    import numpy as np
    import torch
    lib = load_library()
    dev = frames[0].device
    B = len(frames)
    for f in frames:
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.stride(2) != 1 or f.stride(1) != 3 or not f.is_cuda:
            raise ValueError("frames must be uint8 CUDA tensors [H, W, 3] with packed pixels")
    ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64).to(dev)
    dims = torch.tensor([[f.shape[0], f.shape[1], f.stride(0)] for f in frames], dtype=torch.int32).to(dev)
    m = torch.as_tensor(np.asarray(mats, dtype=np.float64).reshape(B, 6)).to(dev)
    out_w, out_h = int(output_size[0]), int(output_size[1])
    out = torch.empty(B, out_h, out_w, 3, dtype=torch.uint8, device=dev)
    rc = lib.capf_warp_affine(_stream(out), _p(ptrs), _p(dims), _p(m), B, out_h, out_w, _p(out))
    if rc:
        raise CapfError(f"capf_warp_affine failed ({rc})")
    return out


ERASE_MAX_PATCHES = 32        # include/capf.h :: capf_erase_patches (the joint cap)


def erase_patches(images_u8, centers, mask=None, size=70, use_mean=True, out=None):
    """capf_erase_patches: erase_image (mvn/utils/img.py:179-198) for a batch.  images_u8: uint8 CUDA [B, H, W, 3]; centers: fp32 CUDA [B, P, 2]
    = (x, y) in crop pixels, P <= 32; mask: uint8 (or bool) CUDA [B, P] or None = every patch; out: None (a new tensor), images_u8 itself (in
    place) or a uint8 tensor of its shape sharing no byte with it.  Every input is contiguous, else ValueError (nothing is copied behind the
    caller's back).  A patch whose centre is NaN or infinite is skipped (the reference raises).  -> out; enqueued on the current stream of
    that device, no synchronisation."""
    import torch
    lib = load_library()
    if images_u8.dim() != 4 or images_u8.shape[-1] != 3 or images_u8.dtype != torch.uint8 or not images_u8.is_cuda or not images_u8.is_contiguous():
        raise ValueError(f"images must be a contiguous uint8 CUDA tensor [B, H, W, 3], not {tuple(images_u8.shape)} {images_u8.dtype} {images_u8.device}")
    B, H, W, _ = images_u8.shape
    dev = images_u8.device
    if centers.dim() != 3 or centers.shape[0] != B or centers.shape[2] != 2 or centers.dtype != torch.float32 or centers.device != dev or not centers.is_contiguous():
        raise ValueError(f"centers must be a contiguous fp32 tensor [{B}, P, 2] on {dev}, not {tuple(centers.shape)} {centers.dtype} {centers.device}")
    P = centers.shape[1]
    if mask is not None:
        if tuple(mask.shape) != (B, P) or mask.dtype not in (torch.uint8, torch.bool) or mask.device != dev or not mask.is_contiguous():
            raise ValueError(f"mask must be a contiguous uint8 / bool tensor [{B}, {P}] on {dev}, not {tuple(mask.shape)} {mask.dtype} {mask.device}")
    if out is None:
        out = torch.empty_like(images_u8)
    elif out.shape != images_u8.shape or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor {tuple(images_u8.shape)} on {dev}, not {tuple(out.shape)} {out.dtype} {out.device}")
    if int(size) < 0:
        raise ValueError(f"size must not be negative, got {size}")
    if B == 0 or P == 0 or H == 0 or W == 0:          # nothing to erase (an empty tensor has no address)
        if out.data_ptr() != images_u8.data_ptr():
            out.copy_(images_u8)
        return out
    need = lib.capf_erase_scratch_bytes(B, P)
    # (freed on return: the caching allocator hands it out again only to work ordered after these kernels on this stream)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    rc = lib.capf_erase_patches(_stream(images_u8), _p(images_u8), B, H, W, _p(centers), _p(mask), P, int(size), 1 if use_mean else 0, _p(out),
                                _p(scratch), need)
    if rc:
        raise CapfError(f"capf_erase_patches failed ({rc})")
    return out


def jpeg_info(data):
    """data: bytes of a JPEG file -> dict(width, height, components, h_samp, v_samp, scratch_bytes); CapfError for what capf_jpeg_decode does
    not take (progressive, arithmetic, CMYK, ...).  Host code, no GPU."""
    lib = load_library()
    w, h, nc, hs, vs, sb = c_int32(), c_int32(), c_int32(), c_int32(), c_int32(), c_size_t()
    rc = lib.capf_jpeg_info(data, len(data), byref(w), byref(h), byref(nc), byref(hs), byref(vs), byref(sb))
    if rc:
        raise CapfError(f"capf_jpeg_info: not a JPEG this path decodes ({rc})")
    return dict(width=w.value, height=h.value, components=nc.value, h_samp=hs.value, v_samp=vs.value, scratch_bytes=sb.value)


def jpeg_coefficients(data):
    """The host half of the decoder: quantised DCT coefficients (natural order) per component, list of int16 numpy arrays
    [block rows, block cols, 64] over the MCU-padded image.  No GPU."""
    import numpy as np
    lib = load_library()
    info = jpeg_info(data)
    hs, vs, nc = info["h_samp"], info["v_samp"], info["components"]
    mx, my = -(-info["width"] // (8 * hs)), -(-info["height"] // (8 * vs))
    shapes = [(my * vs, mx * hs)] + [(my, mx)] * (nc - 1)
    total = sum(a * b * 64 for a, b in shapes)
    buf = np.zeros(total, np.int16)
    rc = lib.capf_jpeg_coefficients(data, len(data), buf.ctypes.data_as(c_void_p), total)
    if rc:
        raise CapfError(f"capf_jpeg_coefficients failed ({rc})")
    out, o = [], 0
    for a, b in shapes:
        out.append(buf[o:o + a * b * 64].reshape(a, b, 64))
        o += a * b * 64
    return out


def jpeg_decode(data, device="cuda"):
    """cv2.imread(..., IMREAD_COLOR) of a baseline JPEG held in memory: bytes -> uint8 CUDA tensor [H, W, 3], BGR (host Huffman decode, GPU
    IDCT / upsampling / colour conversion; bit-exact against libjpeg-turbo's default decode)."""
    import torch
    lib = load_library()
    info = jpeg_info(data)
    out = torch.empty(info["height"], info["width"], 3, dtype=torch.uint8, device=device)
    scratch = torch.empty(info["scratch_bytes"], dtype=torch.uint8, device=device)
    rc = lib.capf_jpeg_decode(_stream(out), data, len(data), _p(out), out.stride(0), _p(scratch), scratch.numel())
    if rc:
        raise CapfError(f"capf_jpeg_decode failed ({rc})")
    return out


def _coef_shapes(width, height, components, h_samp, v_samp):
    mx, my = -(-width // (8 * h_samp)), -(-height // (8 * v_samp))
    return [(my * v_samp, mx * h_samp)] + [(my, mx)] * (components - 1)


def _split_coefficients(buf, shapes):
    out, o = [], 0
    for a, b in shapes:
        out.append(buf[o:o + a * b * 64].reshape(a, b, 64))
        o += a * b * 64
    return out


def jpeg_coefficients_subseq(data, subseq_bytes=0):
    """capf_jpeg_coefficients_subseq: the batched decoder's entropy stage (subsequence lanes, sync rounds, serial fallback) run serially on
    the CPU; same result layout as jpeg_coefficients.  CapfError where the device would flag the file.  No GPU."""
    import numpy as np
    lib = load_library()
    info = jpeg_info(data)
    shapes = _coef_shapes(info["width"], info["height"], info["components"], info["h_samp"], info["v_samp"])
    total = sum(a * b * 64 for a, b in shapes)
    buf = np.zeros(total, np.int16)
    rc = lib.capf_jpeg_coefficients_subseq(data, len(data), buf.ctypes.data_as(c_void_p), total, int(subseq_bytes))
    if rc:
        raise CapfError(f"capf_jpeg_coefficients_subseq failed ({rc})")
    return _split_coefficients(buf, shapes)


def _byte_arrays(datas):
    datas = [bytes(d) for d in datas]
    n = len(datas)
    ptrs = (ctypes.c_char_p * n)(*datas)
    sizes = (c_size_t * n)(*[len(d) for d in datas])
    return datas, ptrs, sizes


def jpeg_batch_info(datas, subseq_bytes=0):
    """-> (list of dict(width, height, components, coef_elems, status) per file, scratch bytes or None when a file is refused).  status is
    0 or the capf_jpeg_info error of a file outside the supported subset.  Host code, no GPU."""
    lib = load_library()
    datas, ptrs, sizes = _byte_arrays(datas)
    n = len(datas)
    info = (c_int32 * (5 * max(n, 1)))()
    sb = c_size_t()
    rc = lib.capf_jpeg_batch_info(n, ptrs, sizes, int(subseq_bytes), info, byref(sb))
    rows = [dict(zip(("width", "height", "components", "coef_elems", "status"), info[5 * i:5 * i + 5])) for i in range(n)]
    return rows, (sb.value if rc == 0 else None)


def jpeg_decode_batch(datas, device="cuda", subseq_bytes=0, coefficients=False):
    """A batch of baseline JPEG files (bytes) decoded in ONE call, Huffman decode included, on the GPU (capf_jpeg_decode_batch) -> (list of
    uint8 CUDA tensors [H, W, 3] BGR, int32 CUDA status tensor [n][, per file the list of int16 CUDA coefficient tensors [rows, cols, 64]
    per component]).  Nothing is synchronised: read `status` (0 = decoded) before trusting a file.  CapfError (nothing enqueued) when a
    file is outside the supported subset."""
    import torch
    lib = load_library()
    datas, ptrs, sizes = _byte_arrays(datas)
    n = len(datas)
    rows, scratch_bytes = jpeg_batch_info(datas, subseq_bytes)
    bad = [i for i, r in enumerate(rows) if r["status"]]
    if bad or scratch_bytes is None:
        raise CapfError(f"capf_jpeg_batch_info: files {bad} are not JPEGs this path decodes ({[rows[i]['status'] for i in bad]})")
    outs = [torch.empty(r["height"], r["width"], 3, dtype=torch.uint8, device=device) for r in rows]
    status = torch.empty(n, dtype=torch.int32, device=device)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=device)
    coef = torch.empty(sum(r["coef_elems"] for r in rows), dtype=torch.int16, device=device) if coefficients else None
    out_ptrs = (c_void_p * n)(*[o.data_ptr() for o in outs])
    pitches = (c_size_t * n)(*[o.stride(0) for o in outs])
    rc = lib.capf_jpeg_decode_batch(_stream(status), n, ptrs, sizes, out_ptrs, pitches, _p(coef), _p(scratch), scratch_bytes, _p(status),
                                    int(subseq_bytes))
    if rc:
        raise CapfError(f"capf_jpeg_decode_batch failed ({rc})")
    # (scratch may be freed on return: the caching allocator hands it out again only to work ordered after these kernels on this stream)
    if not coefficients:
        return outs, status
    coefs, o = [], 0
    for d, r in zip(datas, rows):
        info = jpeg_info(d)
        coefs.append(_split_coefficients(coef[o:o + r["coef_elems"]], _coef_shapes(r["width"], r["height"], r["components"],
                                                                                     info["h_samp"], info["v_samp"])))
        o += r["coef_elems"]
    return outs, status, coefs


def jpeg_crop_rect(width, height, h_samp, v_samp, mat, output_size):
    """capf_jpeg_crop_rect: which part of a width x height JPEG (sampling factors as jpeg_info reports them) a crop with the forward 2x3
    matrix `mat` to output_size = (out_w, out_h) can read -> (pixel_rect [x0, y0, x1, y1), mcu_rect [mx0, my0, mx1, my1)), both all zero
    when the crop lies wholly outside the image.  Host code, no GPU."""
    import numpy as np
    lib = load_library()
    m = (c_double * 6)(*np.asarray(mat, dtype=np.float64).reshape(6).tolist())
    px, mc = (c_int32 * 4)(), (c_int32 * 4)()
    rc = lib.capf_jpeg_crop_rect(int(width), int(height), int(h_samp), int(v_samp), m, int(output_size[0]), int(output_size[1]), px, mc)
    if rc:
        raise CapfError(f"capf_jpeg_crop_rect failed ({rc})")
    return tuple(px), tuple(mc)


def _crop_batch_info(lib, n, ptrs, sizes, m, out_w, out_h, subseq_bytes):
    info = (c_int32 * (13 * max(n, 1)))()
    sb = c_size_t()
    rc = lib.capf_jpeg_crop_batch_info(n, ptrs, sizes, m.ctypes.data_as(c_void_p), out_w, out_h, int(subseq_bytes), info, byref(sb))
    rows = [dict(zip(("width", "height", "components", "coef_elems", "status"), info[13 * i:13 * i + 5]),
                 pixel_rect=tuple(info[13 * i + 5:13 * i + 9]), mcu_rect=tuple(info[13 * i + 9:13 * i + 13])) for i in range(n)]
    return rc, rows, sb.value


def jpeg_crop_batch_info(datas, mats, output_size, subseq_bytes=0):
    """-> (rc, list of dict(width, height, components, coef_elems (kept), status, pixel_rect, mcu_rect) per file, scratch bytes or None
    when rc != 0).  rc is capf_jpeg_crop_batch_info's return value: 0, CAPF_ERR_INVALID for bad arguments, or the capf_jpeg_info error of
    the first file outside the supported subset.  Host code, no GPU."""
    import numpy as np
    lib = load_library()
    datas, ptrs, sizes = _byte_arrays(datas)
    n = len(datas)
    m = np.ascontiguousarray(np.asarray(mats, dtype=np.float64).reshape(n, 6)) if n else np.zeros((1, 6))
    rc, rows, sb = _crop_batch_info(lib, n, ptrs, sizes, m, int(output_size[0]), int(output_size[1]), subseq_bytes)
    return rc, rows, (sb if rc == 0 else None)


def jpeg_decode_crop_batch(datas, mats, output_size, device="cuda", subseq_bytes=0):
    """Files in, affine crops out, in ONE call (capf_jpeg_decode_crop_batch): datas = baseline JPEG files (bytes), mats = [n, 2, 3] float64
    forward matrices, output_size = (out_w, out_h) -> (uint8 CUDA tensor [n, out_h, out_w, 3] with the bits of
    warp_affine(jpeg_decode_batch(datas)[0], mats, output_size), int32 CUDA status tensor [n]).  Only the MCUs a crop reads are transformed;
    no frame is ever materialised.  Nothing is synchronised: read `status` (0 = decoded) before trusting a crop.  CapfError (nothing
    enqueued) when a file is outside the supported subset."""
    import numpy as np
    import torch
    lib = load_library()
    datas, ptrs, sizes = _byte_arrays(datas)
    n = len(datas)
    out_w, out_h = int(output_size[0]), int(output_size[1])
    m = np.ascontiguousarray(np.asarray(mats, dtype=np.float64).reshape(n, 6)) if n else np.zeros((1, 6))
    rc, rows, scratch_bytes = _crop_batch_info(lib, n, ptrs, sizes, m, out_w, out_h, subseq_bytes)
    bad = [i for i, r in enumerate(rows) if r["status"]]
    if bad:
        raise CapfError(f"capf_jpeg_crop_batch_info: files {bad} are not JPEGs this path decodes ({[rows[i]['status'] for i in bad]})")
    if rc:
        raise CapfError(f"capf_jpeg_crop_batch_info failed ({rc})")
    out = torch.empty(n, out_h, out_w, 3, dtype=torch.uint8, device=device)
    status = torch.empty(n, dtype=torch.int32, device=device)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=device)
    rc = lib.capf_jpeg_decode_crop_batch(_stream(out), n, ptrs, sizes, m.ctypes.data_as(c_void_p), out_h, out_w, _p(out), _p(scratch), scratch_bytes,
                                         _p(status), int(subseq_bytes))
    if rc:
        raise CapfError(f"capf_jpeg_decode_crop_batch failed ({rc})")
    # (scratch may be freed on return: the caching allocator hands it out again only to work ordered after these kernels on this stream)
    return out, status


# ---- N2: evaluation metrics (mvn/models/loss.py:25-101, datasets/human36m.py:358-417) ---------------------------
def pose_errors(pred, gt, prev=None):
    """pred / gt: CUDA fp32 [n, J, 3]; prev: CUDA int32 [n] or None (= i-1).  -> CUDA fp32 [n, 4] =
    per-pose {MPJPE, P_MPJPE, N_MPJPE, velocity error}."""
    import torch
    lib = load_library()
    n, J, _ = pred.shape
    err = torch.empty(n, 4, dtype=torch.float32, device=pred.device)
    rc = lib.capf_pose_errors(_stream(pred), _p(pred.contiguous()), _p(gt.contiguous()), n, J, _p(prev), _p(err))
    if rc:
        raise CapfError(f"capf_pose_errors failed ({rc})")
    return err


def segment_sums(err, segment=None, prev=None, n_segments=1):
    """-> (sums float64 [n_segments, 4], counts int32 [n_segments, 2]) on the device."""
    import torch
    lib = load_library()
    n = err.shape[0]
    sums = torch.empty(n_segments, 4, dtype=torch.float64, device=err.device)
    counts = torch.empty(n_segments, 2, dtype=torch.int32, device=err.device)
    rc = lib.capf_segment_sums(_stream(err), _p(err), _p(segment), _p(prev), n, n_segments, _p(sums), _p(counts))
    if rc:
        raise CapfError(f"capf_segment_sums failed ({rc})")
    return sums, counts


PCK_THRESHOLDS = 31     # 0, 5, ..., 150 mm (mpii_compute_3d_pck.m:20)


def pck_counts(pred, gt, root=14, to_mm=1.0, segment=None, n_segments=1):
    """capf_pck_counts.  pred / gt: CUDA fp32 [n, J, 3] in the same unit (to_mm: that unit in mm); segment: CUDA int32 [n] or None.
    -> (counts int32 [n_segments, J, 31], mpjpe_sums float64 [n_segments, J], frames int32 [n_segments]) on the device."""
    import torch
    lib = load_library()
    n, J, _ = gt.shape
    dev = gt.device
    counts = torch.empty(n_segments, J, PCK_THRESHOLDS, dtype=torch.int32, device=dev)
    sums = torch.empty(n_segments, J, dtype=torch.float64, device=dev)
    frames = torch.empty(n_segments, dtype=torch.int32, device=dev)
    if segment is not None:
        segment = segment.to(torch.int32).contiguous()
    pred = pred.contiguous()
    gt = gt.contiguous()
    rc = lib.capf_pck_counts(_stream(gt), _p(pred) if n else c_void_p(0), _p(gt) if n else c_void_p(0), n, J, int(root), float(to_mm),
                             _p(segment), n_segments, _p(counts), _p(sums), _p(frames))
    if rc:
        raise CapfError(f"capf_pck_counts failed ({rc})")
    return counts, sums, frames


PCK2D_MAX_THRESHOLDS = 32


def pck2d_counts(pred, gt, thresholds, norm=None, weight=None, strict=False, segment=None, n_segments=1, out=None):
    """capf_pck2d_counts.  pred / gt: CUDA fp32 [n, J, 2]; thresholds: 1..32 Python floats (host; for the reference's PCKh rule already
    multiplied by headsize, with norm=None); norm: CUDA fp32 [n, 2] per-pose (nx, ny) or None = (1, 1); weight: CUDA fp32 [n, J] or
    None; strict: `<` instead of `<=`; segment: CUDA int32 [n] or None (n_segments 1).  out: None, or (counts, valid, err_sums) to write
    into.  -> (counts int32 [n_segments, K, J], valid int32 [n_segments, J], err_sums float64 [n_segments, J]) on the device; enqueued
    on the current stream of that device, no synchronisation."""
    import torch
    lib = load_library()
    n, J, two = gt.shape
    dev, f32 = gt.device, torch.float32
    thr = [float(t) for t in thresholds]
    K = len(thr)
    if two != 2 or tuple(pred.shape) != (n, J, 2) or pred.dtype != f32 or gt.dtype != f32:
        raise CapfError(f"pred / gt must be fp32 [n, J, 2], not {tuple(pred.shape)} {pred.dtype} / {tuple(gt.shape)} {gt.dtype}")
    if norm is not None and (tuple(norm.shape) != (n, 2) or norm.dtype != f32):
        raise CapfError(f"norm must be fp32 [{n}, 2], not {tuple(norm.shape)} {norm.dtype}")
    if weight is not None:
        weight = weight.reshape(n, J) if weight.numel() == n * J else weight
        if tuple(weight.shape) != (n, J) or weight.dtype != f32:
            raise CapfError(f"weight must be fp32 [{n}, {J}] (or [{n}, {J}, 1]), not {tuple(weight.shape)} {weight.dtype}")
    if segment is not None and (tuple(segment.shape) != (n,) or segment.dtype != torch.int32):
        raise CapfError(f"segment must be int32 [{n}], not {tuple(segment.shape)} {segment.dtype}")
    shapes = ((n_segments, K, J), torch.int32), ((n_segments, J), torch.int32), ((n_segments, J), torch.float64)
    if out is None:
        out = tuple(torch.empty(*s, dtype=d, device=dev) for s, d in shapes)
    for t, (s, d) in zip(out, shapes):
        if tuple(t.shape) != s or t.dtype != d or not t.is_contiguous() or t.device != dev:
            raise CapfError(f"out must be contiguous (counts, valid, err_sums) {[x[0] for x in shapes]} on {dev}, got {tuple(t.shape)} {t.dtype}")
    counts, valid, sums = out
    pred, gt = pred.contiguous(), gt.contiguous()
    norm, weight, segment = (None if t is None else t.contiguous() for t in (norm, weight, segment))
    if n == 0:                     # (an empty tensor has no address; the entry reads none of them and takes NULL for each)
        pred = gt = norm = weight = segment = None
    rc = lib.capf_pck2d_counts(_stream(counts), _p(pred), _p(gt), n, J, _p(norm), _p(weight), (c_double * max(K, 1))(*thr), K,
                               1 if strict else 0, _p(segment), n_segments, _p(counts), _p(valid), _p(sums))
    if rc:
        raise CapfError(f"capf_pck2d_counts failed ({rc})")
    return counts, valid, sums


def keypoints_loss(mode, pred, gt, validity, threshold=0.0, want_grad=False):
    """mode 0 MSE, 1 MSESmooth, 2 MAE (loss.py:104-137).  pred / gt [..., D], validity [..., 1] -> (loss[1], dpred | None)."""
    import torch
    lib = load_library()
    D = pred.shape[-1]
    rows = pred.numel() // D
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty(pred.shape, dtype=torch.float32, device=pred.device) if want_grad else None
    v = validity.to(torch.float32).expand(*pred.shape[:-1], 1).contiguous()
    rc = lib.capf_keypoints_loss(_stream(pred), int(mode), _p(pred.contiguous()), _p(gt.contiguous()), _p(v), rows, D,
                                 float(threshold), _p(loss), _p(dpred))
    if rc:
        raise CapfError(f"capf_keypoints_loss failed ({rc})")
    return loss, dpred


# ---- the remaining pose losses of mvn/models/loss.py: KeypointsL2Loss (:140-147), LimbLengthError (:181-201), UNCERTAINTY (:7-13) ----
LIMB_MAX = 64                     # csrc/kernels.h :: LIMB_MAX
UNCERTAINTY_MAX_SIGMAS = 8        # csrc/kernels.h :: UNCERTAINTY_MAX_SIGMAS


def _loss_operands(what, pred, gt):
    """pred / gt of one shape [..., D], fp32, on the GPU -> (contiguous pred, contiguous gt, rows, D); shapes are judged before devices"""
    import torch
    if tuple(pred.shape) != tuple(gt.shape) or pred.dim() < 1 or pred.numel() == 0:
        raise CapfError(f"{what}: pred and gt must have one non-empty shape [..., D], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if not (pred.is_cuda and gt.is_cuda):
        raise CapfError(f"{what} runs on the MI355X only: got a CPU tensor (no CPU fallback)")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise CapfError(f"{what}: pred and gt must be fp32, got {pred.dtype} and {gt.dtype}")
    D = pred.shape[-1]
    return pred.contiguous(), gt.contiguous(), pred.numel() // D, D


def keypoints_l2_loss(pred, gt, validity, want_grad=False, grad_scale=1.0):
    """capf_keypoints_l2_loss (loss.py:140-147).  pred / gt: CUDA fp32 [..., D]; validity: [..., 1] or [...] (one weight per row).
    -> (loss [1], dpred | None); dpred = grad_scale * dloss/dpred, exactly 0 in a masked row and at pred == gt."""
    import torch
    lib = load_library()
    lead = tuple(pred.shape[:-1])
    if tuple(validity.shape) not in (lead, lead + (1,)):
        raise CapfError(f"keypoints_l2_loss: validity must be {lead + (1,)} (one weight per row), got {tuple(validity.shape)}")
    p, g, rows, D = _loss_operands("keypoints_l2_loss", pred, gt)
    if not validity.is_cuda:
        raise CapfError("keypoints_l2_loss runs on the MI355X only: got a CPU validity mask (no CPU fallback)")
    v = validity.to(torch.float32).contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty(pred.shape, dtype=torch.float32, device=pred.device) if want_grad else None
    rc = lib.capf_keypoints_l2_loss(_stream(pred), _p(p), _p(g), _p(v), rows, D, _p(loss), _p(dpred), float(grad_scale))
    if rc:
        raise CapfError(f"capf_keypoints_l2_loss failed ({rc})")
    return loss, dpred


def limb_table(limbs, joints):
    """a sequence of (a, b) joint pairs -> the host int32 [L, 2] array capf_limb_length_errors takes; refuses what the entry refuses"""
    pairs = [tuple(int(v) for v in pair) for pair in limbs]
    if not 1 <= len(pairs) <= LIMB_MAX or any(len(pair) != 2 for pair in pairs):
        raise CapfError(f"limbs must be 1..{LIMB_MAX} pairs of joints, got {len(pairs)} entries")
    bad = [pair for pair in pairs if not (0 <= pair[0] < joints and 0 <= pair[1] < joints)]
    if bad:
        raise CapfError(f"limb {bad[0]} names a joint outside [0, {joints})")
    return (c_int32 * (2 * len(pairs)))(*[v for pair in pairs for v in pair]), len(pairs)


def limb_length_errors(pred, gt, limbs, want_grad=False, grad_scale=1.0):
    """capf_limb_length_errors (loss.py:181-201 per pose).  pred / gt: CUDA fp32 [n, J, 3], J <= 32; limbs: 1..64 (a, b) pairs (host).
    -> (err fp32 [n, L], dpred | None); dpred [n, J, 3] = grad_scale * d(sum_l err[i, l]) / dpred (exchange pred and gt for the target's)."""
    import torch
    lib = load_library()
    if pred.dim() != 3 or pred.shape[-1] != 3:
        raise CapfError(f"limb_length_errors: pred and gt must be [n, J, 3], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    table, L = limb_table(limbs, pred.shape[1])
    p, g, _, _ = _loss_operands("limb_length_errors", pred, gt)
    n, J, _ = p.shape
    err = torch.empty(n, L, dtype=torch.float32, device=pred.device)
    dpred = torch.empty(n, J, 3, dtype=torch.float32, device=pred.device) if want_grad else None
    rc = lib.capf_limb_length_errors(_stream(pred), _p(p), _p(g), n, J, table, L, _p(err), _p(dpred), float(grad_scale))
    if rc:
        raise CapfError(f"capf_limb_length_errors failed ({rc})")
    return err, dpred


def limb_length_sums(err, segment=None, n_segments=1):
    """capf_limb_length_sums.  err: CUDA fp32 [n, L]; segment: CUDA int32 [n] or None (n_segments 1).
    -> (sums float64 [n_segments, L], counts int64 [n_segments]) on the device; no synchronisation."""
    import torch
    lib = load_library()
    if err.dim() != 2 or err.numel() == 0 or err.dtype != torch.float32:
        raise CapfError(f"limb_length_sums: err must be a non-empty fp32 [n, L], got {tuple(err.shape)} {err.dtype}")
    n, L = err.shape
    if segment is None and n_segments != 1:
        raise CapfError("limb_length_sums: n_segments > 1 needs a segment table")
    if segment is not None and (tuple(segment.shape) != (n,) or segment.dtype != torch.int32):
        raise CapfError(f"limb_length_sums: segment must be int32 [{n}], got {tuple(segment.shape)} {segment.dtype}")
    if not err.is_cuda or (segment is not None and not segment.is_cuda):
        raise CapfError("limb_length_sums runs on the MI355X only: got a CPU tensor (no CPU fallback)")
    sums = torch.empty(n_segments, L, dtype=torch.float64, device=err.device)
    counts = torch.empty(n_segments, dtype=torch.int64, device=err.device)
    seg = None if segment is None else segment.contiguous()
    rc = lib.capf_limb_length_sums(_stream(err), _p(err.contiguous()), _p(seg), n, L, int(n_segments), _p(sums), _p(counts))
    if rc:
        raise CapfError(f"capf_limb_length_sums failed ({rc})")
    return sums, counts


def uncertainty_loss(pred, gt, sigmas, want_dpred=False, want_dsigma=None, grad_scale=1.0):
    """capf_uncertainty_loss (loss.py:7-13).  pred / gt: CUDA fp32 [..., D]; sigmas: 1..8 CUDA fp32 tensors, each [..., D] or [..., 1];
    want_dsigma: None (none) or one bool per sigma.  -> (loss [1], dpred | None, [dsigma_k | None per sigma]); every gradient is
    multiplied by grad_scale, dsigma_k has sigma k's own shape."""
    import torch
    lib = load_library()
    sigmas = list(sigmas)
    K = len(sigmas)
    if not 1 <= K <= UNCERTAINTY_MAX_SIGMAS:
        raise CapfError(f"uncertainty_loss takes 1..{UNCERTAINTY_MAX_SIGMAS} sigma tensors, got {K}")
    lead, D = tuple(pred.shape[:-1]), (pred.shape[-1] if pred.dim() else 0)
    for k, s in enumerate(sigmas):
        if tuple(s.shape) not in (lead + (D,), lead + (1,)):
            raise CapfError(f"uncertainty_loss: sigma {k} must be {lead + (D,)} or {lead + (1,)}, got {tuple(s.shape)}")
    want_dsigma = [False] * K if want_dsigma is None else [bool(w) for w in want_dsigma]
    if len(want_dsigma) != K:
        raise CapfError(f"uncertainty_loss: want_dsigma must have one entry per sigma ({K}), got {len(want_dsigma)}")
    p, g, rows, D = _loss_operands("uncertainty_loss", pred, gt)
    if not all(s.is_cuda for s in sigmas):
        raise CapfError("uncertainty_loss runs on the MI355X only: got a CPU sigma (no CPU fallback)")
    if any(s.dtype != torch.float32 for s in sigmas):
        raise CapfError("uncertainty_loss: every sigma must be fp32")
    sig = [s.contiguous() for s in sigmas]
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty(pred.shape, dtype=torch.float32, device=pred.device) if want_dpred else None
    dsig = [torch.empty(s.shape, dtype=torch.float32, device=pred.device) if w else None for s, w in zip(sig, want_dsigma)]
    ptrs = (c_void_p * K)(*[s.data_ptr() for s in sig])
    widths = (c_int32 * K)(*[s.shape[-1] for s in sig])
    dptrs = (c_void_p * K)(*[d.data_ptr() if d is not None else None for d in dsig])
    rc = lib.capf_uncertainty_loss(_stream(pred), _p(p), _p(g), rows, D, ptrs, widths, K, _p(loss), _p(dpred), dptrs, float(grad_scale))
    if rc:
        raise CapfError(f"capf_uncertainty_loss failed ({rc})")
    return loss, dpred, dsig
