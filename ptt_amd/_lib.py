"""ctypes binding of libptt_hip.so (the C ABI declared in include/ptt_hip.h).

The header is the declaration: it is read once at import, and the list of entry points, their restype / argtypes and the
PTT_* constants all come from it. Only the structures are restated here (tests compare them with what gcc makes of the header).
There is no fallback: if the shared library is missing or fails to load, every op raises.
"""
import ctypes
import os
import re
from ctypes import Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_longlong, c_size_t, c_uint32, c_void_p

from .build import HEADER as HEADER_PATH, LIB as LIB_PATH


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def parse_defines(text):
    """{name: value} of every `#define PTT_NAME <decimal integer>` of a header text."""
    return {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PTT_\w+)[ \t]+(-?\d+)[ \t]*$", _strip_comments(text), re.M)}


# the scalar types the C ABI uses; every pointer (structures included) is passed as c_void_p, which takes byref(structure), a
# ctypes array, a device or host address and None
CTYPES = {"int": c_int, "int32_t": c_int32, "uint32_t": c_uint32, "int64_t": c_int64, "long long": c_longlong, "size_t": c_size_t,
          "float": c_float, "double": c_double, "ptt_stream_t": c_void_p}


def _ctype(decl, name, is_return=False):
    words = decl.replace("*", " * ").split()
    if not is_return and len(words) > 1 and words[-1] != "*":
        words.pop()                                               # the parameter's name
    if "*" in words:
        if not is_return:
            return c_void_p
        if words == ["const", "char", "*"]:
            return c_char_p
    base = " ".join(w for w in words if w != "const")
    if base not in CTYPES:
        raise RuntimeError("ptt_amd: %s of %s in include/ptt_hip.h has the type '%s', which ptt_amd/_lib.py does not map to ctypes"
                           % ("the return value" if is_return else "parameter '%s'" % decl.strip(), name, base))
    return CTYPES[base]


def parse_prototypes(text):
    """{name: (restype, [argtypes])} of every function a header text declares, in its order. The header is plain C: one
    prototype per `;`, `(void)` for no parameters; preprocessor lines, typedefs and the bodies of enums / structures are skipped.
    A statement that is none of these, or a type outside CTYPES, raises."""
    text = re.sub(r"^[ \t]*#.*$", " ", _strip_comments(text), flags=re.M).replace('extern "C" {', " ")
    text = re.sub(r"\{[^{}]*\}", " ", text)
    protos = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split()).lstrip("} ")
        if not stmt or stmt.split()[0] in ("typedef", "enum", "struct"):
            continue
        m = re.fullmatch(r"(.+?)\b(\w+) ?\((.*)\)", stmt)
        if m is None:
            raise RuntimeError("ptt_amd: cannot read '%s' in include/ptt_hip.h as a function prototype" % stmt)
        ret, name, params = m.groups()
        params = [] if params.strip() == "void" else params.split(",")
        protos[name] = (_ctype(ret, name, is_return=True), [_ctype(p, name) for p in params])
    return protos


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError("ptt_amd: %s is missing — the Python binding takes every prototype and constant of the C ABI from it" % HEADER_PATH)
    with open(HEADER_PATH) as fh:
        return fh.read()


_header = _read_header()
PROTOTYPES = parse_prototypes(_header)      # what lib() applies as restype / argtypes
EXPORTS = list(PROTOTYPES)                  # every symbol include/ptt_hip.h declares (tests check the library exports all of them)
DEFINES = parse_defines(_header)
ABI_VERSION = DEFINES["PTT_ABI_VERSION"]
PTT_SA_MAX_LAYERS = DEFINES["PTT_SA_MAX_LAYERS"]
PTT_MAX_SEGMENTS = DEFINES["PTT_MAX_SEGMENTS"]
PTT_CROP_JOBS_BY_VALUE_MAX = DEFINES["PTT_CROP_JOBS_BY_VALUE_MAX"]
PTT_TRAIN_MAX_CANDS = DEFINES["PTT_TRAIN_MAX_CANDS"]
PTT_OPTIM_MAX_GROUPS = DEFINES["PTT_OPTIM_MAX_GROUPS"]
OPTIM_KINDS = {"adam": DEFINES["PTT_OPTIM_ADAM"], "adamw": DEFINES["PTT_OPTIM_ADAMW"], "sgd": DEFINES["PTT_OPTIM_SGD"]}


class CropJob(Structure):
    """ptt_crop_job (include/ptt_hip.h): one crop_center_pc; arrays of these are uploaded to the device."""
    _fields_ = [("points", c_void_p), ("ld", c_int64),
                ("lo1", c_double * 3), ("hi1", c_double * 3), ("trans", c_double * 3), ("rot", c_double * 9),
                ("lo2", c_double * 3), ("hi2", c_double * 3),
                ("out", c_void_p), ("count", c_void_p), ("n_points", c_int32), ("capacity", c_int32),
                ("label_out", c_void_p), ("ltrans", c_double * 3), ("lrot", c_double * 9), ("llo", c_double * 3), ("lhi", c_double * 3),
                ("append", c_int32), ("reserved", c_int32)]


PTT_SCAN_MAX_STEPS = DEFINES["PTT_SCAN_MAX_STEPS"]
SCAN_KINDS = {"rotate": DEFINES["PTT_SCAN_ROTATE"], "translate": DEFINES["PTT_SCAN_TRANSLATE"], "affine": DEFINES["PTT_SCAN_AFFINE"]}


class ScanStep(Structure):
    """ptt_scan_step: one rotate / translate / affine of a scan's way into the reference frame."""
    _fields_ = [("kind", c_int32), ("reserved", c_int32), ("m", c_double * 12)]


class ScanJob(Structure):
    """ptt_scan_job: one raw (n_points, row_floats) scan -> a planar (3, n_points) cloud; device or pinned host memory."""
    _fields_ = [("raw", c_void_p), ("out", c_void_p), ("ld", c_int64), ("n_points", c_int32), ("row_floats", c_int32),
                ("n_steps", c_int32), ("reserved", c_int32), ("steps", ScanStep * PTT_SCAN_MAX_STEPS)]


class PreloadJob(Structure):
    """ptt_preload_job: one crop_pc of a planar cloud in its own frame, planar output; arrays of these are uploaded to the device."""
    _fields_ = [("points", c_void_p), ("ld", c_int64), ("n_points", c_int32), ("capacity", c_int32),
                ("lo", c_double * 3), ("hi", c_double * 3), ("out", c_void_p), ("out_ld", c_int64), ("count", c_void_p)]


class RegularizeJob(Structure):
    """ptt_regularize_job: regularize_pc over the concatenation of up to 4 compacted crops."""
    _fields_ = [("seg", c_void_p * PTT_MAX_SEGMENTS), ("seg_count", c_void_p * PTT_MAX_SEGMENTS),
                ("seg_capacity", c_int32 * PTT_MAX_SEGMENTS), ("out", c_void_p), ("info", c_void_p),
                ("n_seg", c_int32), ("input_size", c_int32)]


class TrackBox(Structure):
    """ptt_track_box: one tracklet's box in float64, quaternion (w, x, y, z); host memory."""
    _fields_ = [("center", c_double * 3), ("wlh", c_double * 3), ("quat", c_double * 4)]


class TrainCand(Structure):
    """ptt_train_cand: one candidate sample of a training batch (its crops' scratch, labels' values and Philox counter words);
    arrays of these are uploaded to the device."""
    _fields_ = [("search", c_void_p), ("label", c_void_p), ("first", c_void_p), ("prev", c_void_p), ("counts", c_void_p),
                ("reg", c_float * 4), ("index", c_uint32), ("epoch", c_uint32), ("capacity", c_int32), ("reserved", c_int32)]


class TrainAug(Structure):
    """ptt_train_aug: one candidate's augmentation map, x' = m00 x + m01 y, y' = m10 x + m11 y, z' = kz z; arrays of these are
    uploaded to the device, parallel to the candidates."""
    _fields_ = [("m", c_float * 4), ("kz", c_float), ("reserved", c_float * 3)]


class TrainBatchDesc(Structure):
    """ptt_train_batch_desc: the outputs and sizes of ptt_train_batch_f32 (passed by value, host memory)."""
    _fields_ = [("search_points", c_void_p), ("template_points", c_void_p), ("cls_label", c_void_p), ("reg_label", c_void_p),
                ("src_out", c_void_p), ("idx_search_out", c_void_p), ("idx_template_out", c_void_p), ("info", c_void_p), ("totals", c_void_p),
                ("B", c_int32), ("n_cand", c_int32), ("search_size", c_int32), ("template_size", c_int32), ("min_points", c_int32),
                ("seed_lo", c_uint32), ("seed_hi", c_uint32), ("reserved", c_int32)]


class BnTrainTail(Structure):
    """ptt_bn_train_tail: a training-mode BatchNorm's bookkeeping, done by the launch that forms the statistics."""
    _fields_ = [("gamma", c_void_p), ("beta", c_void_p), ("act_a", c_void_p), ("act_b", c_void_p),
                ("running_mean", c_void_p), ("running_var", c_void_p), ("num_batches_tracked", c_void_p), ("momentum", c_float)]


class BnBwdInput(Structure):
    """ptt_bn_bwd_input: a layer's BatchNorm + ReLU backward as the A operand of ptt_rows_gemm_bnbwd_fused_f32."""
    _fields_ = [("g", c_void_p), ("ldg", c_int), ("arg", c_void_p), ("ns", c_int), ("z", c_void_p), ("ldz", c_int),
                ("k1", c_void_p), ("c0", c_void_p), ("c1", c_void_p), ("mean", c_void_p), ("act_a", c_void_p), ("act_b", c_void_p),
                ("dz_out", c_void_p), ("ldd", c_int)]


class PackJob(Structure):
    """ptt_pack_job: one weight (view) of ptt_pack_weights_f32; arrays of these are uploaded to the device."""
    _fields_ = [("W", c_void_p), ("out_offset", c_int64), ("stride_out", c_int64), ("stride_k", c_int64),
                ("Cout", c_int32), ("K", c_int32)]


class RowJob(Structure):
    """ptt_row_job: one row-wise layer of ptt_row_jobs_f32 (passed by value, host memory)."""
    _fields_ = [("X", c_void_p), ("X2", c_void_p), ("Xmax", c_void_p), ("Wpacked", c_void_p), ("scale", c_void_p), ("shift", c_void_p),
                ("res", c_void_p), ("res2", c_void_p), ("out", c_void_p), ("out2", c_void_p), ("raw", c_void_p),
                ("rel", c_void_p), ("w1", c_void_p), ("qkv", c_void_p), ("knn", c_void_p), ("pos", c_void_p),
                ("rows", c_int32), ("K", c_int32), ("K1", c_int32), ("ldx", c_int32), ("ldx2", c_int32), ("Cout", c_int32),
                ("act", c_int32), ("res_split", c_int32), ("ldr", c_int32), ("ldr2", c_int32), ("out_split", c_int32),
                ("out_col0", c_int32), ("ldo", c_int32), ("ldo2", c_int32), ("ldraw", c_int32),
                ("prologue", c_int32), ("epilogue", c_int32), ("ldq", c_int32), ("q_off", c_int32), ("k_off", c_int32),
                ("v_off", c_int32), ("ldp", c_int32), ("N", c_int32), ("sm_scale", c_float), ("col_tiles", c_int32),
                ("idx", c_void_p), ("xyz", c_void_p), ("centres", c_void_p), ("wx", c_void_p), ("radius", c_float),
                ("ns", c_int32), ("M", c_int32), ("normalize_xyz", c_int32), ("pro_relu", c_int32)]


class PointJob(Structure):
    """ptt_point_job: one ball-query level or kNN of ptt_point_jobs_f32."""
    _fields_ = [("xyz", c_void_p), ("centre_sel", c_void_p), ("point_sel", c_void_p), ("new_xyz", c_void_p), ("idx64_out", c_void_p),
                ("idx_out", c_void_p), ("rel_out", c_void_p), ("kind", c_int32), ("sel_ld", c_int32), ("B", c_int32),
                ("Nraw", c_int32), ("Npts", c_int32), ("M", c_int32), ("nsample", c_int32), ("radius", c_float)]


class TrackLossDesc(Structure):
    """ptt_track_loss_desc: the inputs of the four tracking losses (passed by value, host memory)."""
    _fields_ = [("seed_cls", c_void_p), ("cls_label", c_void_p), ("search_inds", c_void_p), ("votes", c_void_p), ("reg_label", c_void_p),
                ("box_data", c_void_p), ("centres", c_void_p), ("pos_weight_seed", c_void_p), ("pos_weight_box", c_void_p),
                ("B", c_int32), ("N", c_int32), ("Ns", c_int32), ("M", c_int32), ("ld_reg", c_int32),
                ("w_seed_cls", c_float), ("w_seed_reg", c_float), ("w_box_cls", c_float), ("w_box_reg", c_float)]


class AdamTensor(Structure):
    """ptt_adam_tensor: one parameter with its gradient and moments; arrays of these are uploaded to the device."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("n", c_int64)]


class GradJob(Structure):
    """ptt_grad_job: one contribution to a parameter gradient (row-chunk partial sums); arrays of these are uploaded to the device."""
    _fields_ = [("partial", c_void_p), ("nchunks", c_int32), ("reserved", c_int32)]


class GradSegment(Structure):
    """ptt_grad_segment: one destination inside the flat gradient buffer with its jobs."""
    _fields_ = [("dst", c_int64), ("n", c_int32), ("cols", c_int32), ("ld", c_int32), ("job0", c_int32), ("njobs", c_int32), ("out", c_int32),
                ("vec", c_int32), ("reserved", c_int32)]


class AdamHyper(Structure):
    """ptt_adam_hyper (passed by value, host memory)."""
    _fields_ = [("beta1", c_float), ("beta2", c_float), ("one_minus_beta1", c_float), ("one_minus_beta2", c_float), ("eps", c_float), ("step_size", c_float), ("bias2_sqrt", c_float),
                ("weight_decay", c_float), ("max_norm", c_float), ("write_clipped", c_int32)]


class OptimTensor(Structure):
    """ptt_optim_tensor: one parameter with its gradient, its optimizer state and its group; arrays of these are uploaded to the device."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("state1", c_void_p), ("state2", c_void_p), ("n", c_int64),
                ("group", c_int32), ("reserved", c_int32)]


class OptimHyper(Structure):
    """ptt_optim_hyper: one parameter group's hyper-parameters (arrays of these: host memory, or device memory in the _dev form)."""
    _fields_ = [("kind", c_int32), ("first_step", c_int32), ("beta1", c_float), ("beta2", c_float), ("one_minus_beta1", c_float),
                ("one_minus_beta2", c_float), ("eps", c_float), ("step_size", c_float), ("bias2_sqrt", c_float), ("weight_decay", c_float),
                ("decay", c_float), ("reserved", c_int32)]


class SaLayer(Structure):
    _fields_ = [("Wpacked", c_void_p), ("scale", c_void_p), ("shift", c_void_p),
                ("Cin", c_int), ("Cout", c_int), ("relu", c_int)]


class SaDesc(Structure):
    _fields_ = [("xyz", c_void_p), ("new_xyz", c_void_p), ("idx", c_void_p), ("feat", c_void_p),
                ("feat_sb", c_int64), ("feat_sc", c_int64), ("feat_sn", c_int64),
                ("out", c_void_p), ("out_sb", c_int64), ("out_sc", c_int64), ("out_sm", c_int64),
                ("B", c_int), ("N", c_int), ("M", c_int), ("nsample", c_int), ("C", c_int),
                ("radius", c_float), ("use_xyz", c_int), ("normalize_xyz", c_int), ("n_layers", c_int),
                ("layers", SaLayer * PTT_SA_MAX_LAYERS),
                ("l0_point_term", c_void_p), ("l0_xyz_weight", c_void_p), ("l0_channels", c_int), ("l0_relu", c_int),
                ("compact_ws", c_void_p), ("compact_ws_bytes", c_size_t)]


class XcorrDesc(Structure):
    _fields_ = [("cos_t", c_void_p), ("P", c_void_p), ("w_sim", c_void_p), ("scale0", c_void_p), ("shift0", c_void_p),
                ("out", c_void_p), ("out_sb", c_int64), ("out_sc", c_int64), ("out_sn", c_int64),
                ("sim_out", c_void_p),
                ("B", c_int), ("Ns", c_int), ("Nt", c_int), ("C0", c_int),
                ("n_layers", c_int), ("layers", SaLayer * PTT_SA_MAX_LAYERS),
                ("split", c_int32), ("out_sh", c_int64), ("search_feat", c_void_p), ("templ_feat", c_void_p),
                ("s_sb", c_int64), ("s_sn", c_int64), ("t_sb", c_int64), ("t_sn", c_int64), ("C", c_int), ("eps", c_float)]


class AttnDesc(Structure):
    _fields_ = [("xyz", c_void_p), ("rel", c_void_p), ("knn", c_void_p), ("qkv", c_void_p),
                ("Wd1p", c_void_p), ("Wd2p", c_void_p), ("bd2", c_void_p),
                ("Wg1p", c_void_p), ("bg1", c_void_p), ("Wg2p", c_void_p), ("bg2", c_void_p),
                ("res", c_void_p), ("attn", c_void_p),
                ("B", c_int), ("N", c_int), ("k", c_int), ("D", c_int), ("order", c_void_p), ("heads", c_int)]


class AttnSplitDesc(Structure):
    """ptt_attn_split_desc: ptt_attn_desc without `heads`, Wd2s / Wg1s / Wg2s being split-bf16 packs."""
    _fields_ = [("xyz", c_void_p), ("rel", c_void_p), ("knn", c_void_p), ("qkv", c_void_p),
                ("Wd1p", c_void_p), ("Wd2s", c_void_p), ("bd2", c_void_p),
                ("Wg1s", c_void_p), ("bg1", c_void_p), ("Wg2s", c_void_p), ("bg2", c_void_p),
                ("res", c_void_p), ("attn", c_void_p),
                ("B", c_int), ("N", c_int), ("k", c_int), ("D", c_int), ("order", c_void_p)]


class SaSplitDesc(Structure):
    """ptt_sa_split_desc: the dense SA1 / SA2 stream level in split-bf16 arithmetic (W1s / W2s are split-bf16 packs)."""
    _fields_ = [("xyz", c_void_p), ("new_xyz", c_void_p), ("idx", c_void_p),
                ("l0_point_term", c_void_p), ("l0_xyz_weight", c_void_p), ("l0_relu", c_int),
                ("W1s", c_void_p), ("shift1", c_void_p), ("W2s", c_void_p), ("shift2", c_void_p), ("relu2", c_int),
                ("out", c_void_p), ("out_sb", c_longlong), ("out_sc", c_longlong), ("out_sm", c_longlong),
                ("B", c_int), ("N", c_int), ("M", c_int), ("radius", c_float), ("normalize_xyz", c_int)]


class XcorrSplitDesc(Structure):
    """ptt_xcorr_split_desc: CosineSimAug's two 256 -> 256 layers in split-bf16 arithmetic (W1s / W2s are split-bf16 packs)."""
    _fields_ = [("cos_t", c_void_p), ("P", c_void_p), ("w_sim", c_void_p),
                ("W1s", c_void_p), ("shift1", c_void_p), ("W2s", c_void_p), ("shift2", c_void_p), ("relu2", c_int),
                ("out", c_void_p), ("out_sb", c_longlong), ("out_sc", c_longlong), ("out_sn", c_longlong),
                ("B", c_int), ("Ns", c_int), ("Nt", c_int)]


_lib = None


def lib():
    """Load libptt_hip.so once. Raises RuntimeError (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "ptt_amd: %s is missing — build it with `python -m ptt_amd.build` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        # torch must initialise ITS bundled HIP runtime first: libptt_hip.so then binds to the
        # libamdhip64 already in the process instead of pulling a second copy from /opt/rocm.
        import torch  # noqa: F401
        try:
            loaded = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # e.g. no ROCm runtime on this host
            raise RuntimeError("ptt_amd: cannot load %s: %s" % (LIB_PATH, e))
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(loaded, name)
            fn.restype, fn.argtypes = restype, argtypes
        if loaded.ptt_version() != ABI_VERSION:
            raise RuntimeError("ptt_amd: %s has ABI version %d, this package expects %d — rebuild it with "
                               "`python -m ptt_amd.build`" % (LIB_PATH, loaded.ptt_version(), ABI_VERSION))
        _lib = loaded
    return _lib


def check(rc, what):
    if rc != 0:
        l = lib()
        raise RuntimeError("%s failed: %s (%s)" % (what, l.ptt_error_name(rc).decode(),
                                                   l.ptt_last_error_string().decode()))
