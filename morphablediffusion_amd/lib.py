"""ctypes binding of libmvd_hip.so (C ABI in include/mvd.h: load() derives every restype / argtypes from that header).

The HIP library is the product path: there is NO CPU / PyTorch fallback.  If the shared object is missing
(or fails to load) every entry point raises, loudly.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# MVD_DTYPE (read once, at the first load): "f16" (default) -> libmvd_hip.so, "bf16" -> libmvd_hip_bf16.so, the same sources
# built with bfloat16 MFMA operands and storage (csrc/common.h MVD_BF16; `make -C csrc bf16`): the training dtype of BASELINE
# configs[3].  One process uses one of them.  MVD_LIB_PATH: A/B timing of two builds of the same ABI (development aid).
DTYPE = os.environ.get("MVD_DTYPE", "f16")
if DTYPE not in ("f16", "bf16"):
    raise ValueError(f"MVD_DTYPE must be f16 or bf16, not {DTYPE!r}")
LIB_PATH = os.environ.get("MVD_LIB_PATH", os.path.join(_HERE, "libmvd_hip.so" if DTYPE == "f16" else "libmvd_hip_bf16.so"))

HEADER = os.path.join(_HERE, "..", "include", "mvd.h")


class MvdError(RuntimeError):
    pass


_CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "long": C.c_long, "size_t": C.c_size_t, "float": C.c_float,
           "const char*": C.c_char_p}


def _ctype(decl, func, is_return=False):
    """ctypes type of one C type as include/mvd.h spells it (a parameter with its name, or a return type)."""
    decl = re.sub(r"\s*\*\s*", "* ", decl).strip()  # "const float* const* K", "mvd_ctx** out", "int", "const char*"
    ty = decl if is_return or " " not in decl else decl.rsplit(" ", 1)[0].strip()
    if ty == "void" and is_return:
        return None
    if ty in _CTYPES:
        return _CTYPES[ty]
    if ty.endswith("*"):
        return C.c_void_p
    raise MvdError(f"include/mvd.h: {func}: no ctypes type for {ty!r} (in {decl!r})")


def parse_header(path=HEADER):
    """{name: (restype, [argtypes])} of every function include/mvd.h declares: the ONE place an entry point's signature is
    written (c_api.hip, c_api_morph.hip, c_api_hooks.hip and engine_train.hip, which define them, are compiled against the same header).  The
    header keeps to one declaration style -- `RET name(ARGS);`, no macros in signatures, `(void)` for an empty list -- so this
    is a regular expression, not a C parser; a type outside the table above raises MvdError."""
    try:
        with open(path) as fh:
            text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    except OSError as e:
        raise MvdError(f"cannot read the C ABI header {path}: {e}")
    protos = {}
    for ret, name, args in re.findall(r"([\w \t\*]+?)\b(mvd_\w+)\s*\(([^()]*)\)\s*;", text):
        args = [] if args.strip() == "void" else args.split(",")
        protos[name] = (_ctype(ret, name, is_return=True), [_ctype(a, name) for a in args])
    if not protos:
        raise MvdError(f"{path} declares no mvd_* function")
    return protos


PROTOTYPES = parse_header()
SYMBOLS = list(PROTOTYPES)  # every entry point of the C ABI, in header order


def csrc_sha16():
    """First 16 hex digits of the SHA-256 over the library's sources (csrc/*.hip, *.h, Makefile, include/mvd.h, sorted by name):
    the build a measurement belongs to.  tools/pmc_traffic.py stamps it into profiles/pmc_traffic.json and bench.py reports
    roofline.traffic only when the stamp matches the tree it runs from."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h")) +
                   [os.path.join(_HERE, "csrc", "Makefile"), os.path.join(_HERE, "..", "include", "mvd.h")])
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


class UNetConfigC(C.Structure):
    _fields_ = [("image_size", C.c_int), ("in_channels", C.c_int), ("out_channels", C.c_int),
                ("model_channels", C.c_int), ("num_res_blocks", C.c_int), ("channel_mult", C.c_int * 4),
                ("num_heads", C.c_int), ("context_dim", C.c_int), ("volume_dims", C.c_int * 4),
                ("attention_levels", C.c_int)]


class VolumeConfigC(C.Structure):
    _fields_ = [("time_dim", C.c_int), ("view_dim", C.c_int), ("num_views", C.c_int), ("input_image_size", C.c_int),
                ("frustum_volume_depth", C.c_int), ("spatial_volume_size", C.c_int),
                ("spatial_volume_length", C.c_float), ("frustum_volume_length", C.c_float), ("projection", C.c_int),
                ("frustum_dims", C.c_int * 4), ("voxel_size", C.c_float)]


_lib = None


def load():
    """Loads libmvd_hip.so; raises MvdError if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MvdError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       f"(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        if not hasattr(lib, name):
            raise MvdError(f"libmvd_hip.so does not export {name}")
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if "MVD_LIB_PATH" not in os.environ and lib.mvd_compute_dtype().decode() != DTYPE:
        raise MvdError(f"{LIB_PATH} computes in {lib.mvd_compute_dtype().decode()}, MVD_DTYPE asks for {DTYPE}")
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise MvdError(load().mvd_last_error().decode())


def ptr(t):
    """Device/host pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "tensor must be contiguous at the C boundary"
    return t.data_ptr()
