"""ctypes binding of ``liba3vt.so`` (the C ABI declared in ``include/a3vt.h``).

There is deliberately NO fallback: if the shared library is missing or a call fails, a
``RuntimeError`` is raised.  ``build()`` compiles the HIP sources in-tree with hipcc for gfx950.
"""
import ctypes
import glob
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("A3VT_LIB", os.path.join(_HERE, "liba3vt.so"))  # A3VT_LIB: another build of the library (tools/asan_host.sh)
SOURCES = ["capi.hip", "gcn_gemm.hip", "gcn_gemmw.hip", "gcn_dww.hip", "gcn_gemm16.hip", "gcn_gemm3.hip", "gcn_csr.hip", "gcn_csrq.hip", "gcn_csrqs.hip", "gcn_bf16s.hip", "posenc.hip", "posenc_wide.hip", "bias_grad.hip", "bnrelu.hip", "conv5.hip", "conv5f.hip", "adam.hip", "sample.hip", "chamfer.hip", "nn_prune.hip",
           "pooling.hip", "fold.hip", "ddqn.hip", "qnet_input.hip", "latent_nn.hip", "latent_policy.hip", "ddqn_latent.hip",
           "candidate_tally.hip", "touch_render.hip", "voxel.hip", "scene_render.hip", "touch_assemble.hip", "chart_head.hip",
           "touch_pack.hip", "grasp_close.hip", "hull_place.hip", "posed_render.hip"]
# Per-file extra flags (none at present; sample.hip / gcn_csr.hip rely on IEEE NaN semantics — the reference's NaN
# scrubs, a3vt_check_finite — so fast-math style flags must never be applied globally).
# chamfer.hip: keep the nearest-neighbour loop on scalar fp32 ops (the SLP vectoriser would re-pack it into v_pk_*_f32,
# which issues at half the rate on gfx950 and needs s_nop hazard padding)
# gcn_csrq.hip: scalar fma chains keep one register per edge weight (v_pk_fma_f32 wants (w, w) pairs): see the file header
# voxel.hip: no multiply-add may be fused: its grids equal the reference's bit for bit (the steps are spelled with __f*_rn as well)
# grasp_close.hip: no multiply-add may be fused: the LDS walk and the global-memory walk of a query must give the same booleans
# hull_place.hip: no multiply-add may be fused: ops.py's float64 NumPy form of the rule states the same operations in the same order
EXTRA_FLAGS = {"chamfer.hip": ["-fno-slp-vectorize"], "nn_prune.hip": ["-fno-slp-vectorize"],
               "gcn_csrq.hip": ["-fno-slp-vectorize"], "gcn_csrqs.hip": ["-fno-slp-vectorize"],
               "voxel.hip": ["-ffp-contract=off"], "grasp_close.hip": ["-ffp-contract=off"],
               "hull_place.hip": ["-ffp-contract=off"],
               "gcn_gemmw.hip": ["-std=c++20"], "gcn_dww.hip": ["-std=c++20"]}   # (templated lambdas over the chunk / column-tile index)

_vp, _i, _sz, _u64, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_float


class AdjSplit(ctypes.Structure):
    """``a3vt_adj_split`` (include/a3vt.h): the fused vision + touch adjacency as P + a complete bipartite block."""
    _fields_ = [("rowptr", _vp), ("col", _vp), ("scale", _vp), ("cls", _vp),
                ("max_degree", ctypes.c_int32), ("n_seam", ctypes.c_int32), ("n_centre", ctypes.c_int32)]


class MlpLayer(ctypes.Structure):
    """``a3vt_mlp_layer`` (include/a3vt.h): one Linear of a layer table, weight in torch's [out][in] layout."""
    _fields_ = [("weight", _vp), ("bias", _vp), ("n_in", ctypes.c_int32), ("n_out", ctypes.c_int32), ("relu", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class Mlp(ctypes.Structure):
    """``a3vt_mlp``: the layer table of ``a3vt_latent_policy_fwd`` / ``_bwd``."""
    _fields_ = [("layer", MlpLayer * 16), ("n_layers", ctypes.c_int32), ("concat_at", ctypes.c_int32), ("latent_size", ctypes.c_int32),
                ("transform", ctypes.c_int32), ("scale", ctypes.c_float), ("offset", ctypes.c_float)]


class MlpGrads(ctypes.Structure):
    """``a3vt_mlp_grads``: where ``a3vt_latent_policy_bwd`` writes (or adds) each layer's gradients."""
    _fields_ = [("dweight", _vp * 16), ("dbias", _vp * 16)]


_SCALARS = {"int": _i, "size_t": _sz, "float": _f, "double": ctypes.c_double, "long long": ctypes.c_longlong, "uint64_t": _u64}


def parse_header(text):
    """``name -> (restype, [argtypes])`` of every prototype ``RET a3vt_name(ARGS);`` in the text of a C header.

    Anything with ``*`` is a ``c_void_p`` (the struct pointers too), a ``const char *`` return a ``c_char_p``; scalars go through
    ``_SCALARS``.  A declaration outside that raises ``ValueError`` and names it: a binding is never guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)                        # comments
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)                               # preprocessor lines
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{[^{}]*\}\s*\w+\s*;", " ", text)         # the struct definitions
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", text)                                  # the extern "C" block's braces
    sigs = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(.*?)\b(a3vt_\w+) ?\((.*)\)", decl)
        if m is None:
            raise ValueError(f"a3vt.h: not a prototype: {decl!r}")
        ret, name, params = m.groups()

        def ctype(words, what):
            if words not in _SCALARS:
                raise ValueError(f"a3vt.h: {name}: no ctypes mapping for {what} in {decl!r}")
            return _SCALARS[words]
        if "(" in params or ")" in params or "[" in params:
            raise ValueError(f"a3vt.h: {name}: cannot split the parameter list of {decl!r}")
        if "*" in ret:
            if ret.split() != ["const", "char", "*"]:
                raise ValueError(f"a3vt.h: {name}: no ctypes mapping for the return type {ret.strip()!r} in {decl!r}")
            res = ctypes.c_char_p
        else:
            res = ctype(ret.strip(), f"the return type {ret.strip()!r}")
        args = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            words = [w for w in param.split() if w != "const"]          # "TYPE name": every parameter is named
            args.append(_vp if "*" in param else ctype(" ".join(words[:-1]), f"parameter {param.strip()!r}"))
        sigs[name] = (res, args)
    return sigs


HEADER = os.path.join(_HERE, "..", "include", "a3vt.h")
with open(HEADER) as _h:
    SIGNATURES = parse_header(_h.read())    # at import: tests read the table before load()

_LIB = None


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -shared → liba3vt.so next to this file (cross-compiles without a GPU)."""
    return _build(force, verbose, LIB_PATH, os.path.join(_HERE, "build"))


def _build(force, verbose, lib_path, objdir):
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    deps = srcs + glob.glob(os.path.join(CSRC, "*.h")) + [HEADER]
    force = force or os.environ.get("A3VT_FORCE_BUILD", "0") not in ("", "0")   # prove on any box that it compiles
    if not force and os.path.exists(lib_path) and all(
            os.path.getmtime(lib_path) >= os.path.getmtime(d) for d in deps if os.path.exists(d)):
        return lib_path
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    common = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC"]
    os.makedirs(objdir, exist_ok=True)
    procs = []
    for name in SOURCES:
        obj = os.path.join(objdir, name.replace(".hip", ".o"))
        cmd = [hipcc, *common, *EXTRA_FLAGS.get(name, []), "-c", os.path.join(CSRC, name), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd), obj))
    objs = []
    for cmd, pr, obj in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
        objs.append(obj)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", lib_path]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return lib_path


def load():
    """Load the library (once).  Raises RuntimeError when it has not been built — no fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"a3vt: native library {LIB_PATH} is missing. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). There is no CPU fallback.")
        # torch first: its wheel bundles its own libamdhip64.so (same SONAME as /opt/rocm's).  The process must
        # hold ONE HIP runtime, and it has to be the one torch initialises, or device pointers / streams handed
        # over from torch mean nothing here ("no ROCm-capable device is detected" otherwise).
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError here = header and library out of sync
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def check(rc, what):
    if rc != 0:
        msg = load().a3vt_last_error()
        raise RuntimeError(f"a3vt: {what} failed (rc={rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device/host pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())
