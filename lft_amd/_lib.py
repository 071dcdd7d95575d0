"""ctypes binding of liblft_hip.so (C ABI declared in include/lft_hip.h) and its in-tree build.

The product path has NO CPU fallback: if the library is missing or fails to load, every entry
point raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or ``build()`` here.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("LFT_LIB_PATH") or os.path.join(HERE, "liblft_hip.so")   # LFT_LIB_PATH: experiment builds (tools/ab_build.py)
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cuh")))     # every source of the library, under CSRC


def _header_text(header: str) -> str:
    """include/<header> without its comments."""
    with open(os.path.join(HERE, "..", "include", header)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


# The integer constants of include/lft_hip.h under their names without the LFT_ prefix: ABI_VERSION (lib() refuses a library that
# reports another one), STATUS_NONFINITE, NUM_PARAMS, PREC_*, MATH_*, ERR_*, LOSS_*, BLOCK_*, LF_*, MAPS_*, GRAD_BUCKETS,
# DISPARITY_AIF, GUARD_MAX_SEGMENTS.
globals().update({k: int(v) for k, v in re.findall(r"^#define LFT_(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", _header_text("lft_hip.h"), flags=re.M)})
# The headers added beside ABI 5 (lft_version unchanged), each with the prefix of its constants: VIEW_NEAR_LARGER, VIEW_NEAR_SMALLER,
# VIEW_MAX_REACH, VIEW_MAX_FILL; SGM_MAX_D; VIS_MASK_VIEWS; OCC_MAX_SUBSETS; lft_hip_aif.h (AIF_) defines none; SHEAR_MAX; BLEND_MAX_PZ;
# FIELD_MAX_VIEWS; REFINE_MAX_VIEWS, REFINE_MAX_RADIUS, REFINE_MAX_FILL, REFINE_TABLE; FOCAL_MAX_D.
ADDON_HEADERS = {"lft_hip_views.h": "VIEW_", "lft_hip_sgm.h": "SGM_", "lft_hip_visibility.h": "VIS_", "lft_hip_occlusion.h": "OCC_", "lft_hip_aif.h": "AIF_",
                 "lft_hip_shear.h": "SHEAR_", "lft_hip_blend.h": "BLEND_", "lft_hip_field.h": "FIELD_", "lft_hip_refine.h": "REFINE_", "lft_hip_focal.h": "FOCAL_"}
for _header, _prefix in ADDON_HEADERS.items():
    globals().update({k: int(v) for k, v in re.findall(r"^#define LFT_(%s\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$" % _prefix, _header_text(_header), flags=re.M)})

_lib = None


class LftError(RuntimeError):
    pass


def _stamp_path(lib_path: str) -> str:
    d, _ = _objects(lib_path)
    return os.path.join(d, os.path.basename(lib_path) + ".flags")


def _flags_stamp() -> str:
    """What the library was built with: the compile / link commands themselves (the flags live in this file, not in a source
    the mtime check sees)."""
    return "\n".join(" ".join(c) for c in build_commands("hipcc", "liblft_hip.so"))


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(HERE, "..", "include", h) for h in ("lft_hip.h", "lft_hip_test.h", *ADDON_HEADERS)]
    if any(os.path.getmtime(d) > t for d in deps):
        return True
    # a change of compiler flags must rebuild too; a shipped library without a stamp (the GPU box gets the .so, not the
    # build directory) is taken as current -- its ABI version is still checked at load time
    stamp = _stamp_path(LIB_PATH)
    return os.path.exists(stamp) and open(stamp).read() != _flags_stamp()


def build(force: bool = False, verbose: bool = False) -> str:
    """hipcc cross-compiles for gfx950 (works without a GPU)."""
    if not force and not needs_build():
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for cmd in build_commands(hipcc, LIB_PATH):
        if verbose:
            print(" ".join(cmd))
    compile_and_link(hipcc, LIB_PATH)
    with open(_stamp_path(LIB_PATH), "w") as f:
        f.write(_flags_stamp())
    return LIB_PATH


# The library's translation units, in build order (csrc/<unit>.hip; the longest compile first, they run in parallel):
#   lft_network      the network: the inference path with its per-stage test entry points, the fp32 training step and the
#                    attention maps from its tape; lft_version / lft_last_error.  One unit, not two: see the file's header
#   lft_lightfield   scene tiling, dihedral transforms, view metrics, data preparation, colour, refocus, disparity, view synthesis
#                    with and without the visibility test, semi-global aggregation, the sweep's occlusion-aware cost, the all-in-focus
#                    image from the winning partial aperture, scene tiling with a per-patch integer shear, windowed blending of
#                    overlapping SR patches, angular tiling of a U x V field, the refinement of a selected disparity map (check, fill, weighted median)
#   lft_objective    losses (the focal-stack term and the adjoint of refocus among them), Adam, the guarded step, the EMA
# A unit emits the kernels of the headers it includes, so each includes only what it launches from.
UNITS = ("lft_network", "lft_lightfield", "lft_objective")
INFERENCE_UNIT = "lft_network"          # where the forward's kernels are (tools/isa_mix.py, the listing the hazard tests mutate)
# The kernels emitted by more than one unit (fragments of their mangled names), with who launches each: none.  The kernels that
# inference and training both launch -- k_conv0<float>, k_pack<float>, k_assemble_t<2> and <4> -- are emitted once, since the two
# share lft_network; the other units share no launch with it or with each other (tests/test_host.py asserts exactly this set).
SHARED_KERNELS = ()
# Flags of every unit.
# -amdgpu-schedule-relaxed-occupancy: the kernels' occupancy is set by their LDS footprint and launch bounds, so the
#   scheduler may spend registers on a better instruction order (+1.2 %, k_spa1 43 -> 41 us event-timed); no arithmetic changes.
# -fno-slp-vectorize: hipcc's SLP pass packs neighbouring scalar f32 operations into v_pk_*_f32, which issue slower beside
#   MFMAs than the two scalar instructions (+1.4 % on the inference bench).  Until round 3 the training code kept the default
#   because the pass also decides which fp32 multiply-adds get contracted, enough to flip a ReLU unit in the screened-seed
#   gradient test; the kink-aligned gradient tests (tests/test_gpu_train.py) pass with and without the flag, so the flags
#   are no longer pinned by a test and every unit uses the same set.
COMMON_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-schedule-relaxed-occupancy=true", "-fPIC", "-fno-slp-vectorize"]


def _objects(lib_path):
    d = os.path.join(os.path.dirname(lib_path), "_build")
    return d, {u: os.path.join(d, os.path.basename(lib_path) + f".{u}.o") for u in UNITS}


def unit_commands(hipcc, form, out, extra=()):
    """One compile line per unit, {unit: command}, all with COMMON_FLAGS.  form "object": the build, out(unit) the object file;
    "listing": the device assembly of the product (hipcc -S) to out(unit); "device": device-only with the caller's `extra`
    arguments (which say what to emit) to out(unit)."""
    mode = {"object": ["-c"], "listing": ["--cuda-device-only", "-S"], "device": ["--cuda-device-only"]}[form]
    return {u: [hipcc, *COMMON_FLAGS, *extra, *mode, os.path.join(CSRC, u + ".hip"), "-o", out(u)] for u in UNITS}


def run_parallel(cmds):
    """Run the commands at the same time (one per unit: four processes); raises LftError with the compiler output of the first
    that failed."""
    procs = [subprocess.Popen(c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for c in cmds]
    outs = [p.communicate()[0] for p in procs]
    for p, o, c in zip(procs, outs, cmds):
        if p.returncode != 0:
            raise LftError("hipcc failed: " + " ".join(c) + "\n" + o)


def listings(isa_dir, hipcc="/opt/rocm/bin/hipcc", reuse=False, extra=()):
    """{unit: path} of the device assembly listings of the product build, isa_dir/<unit>.s; reuse: keep the ones already there."""
    os.makedirs(isa_dir, exist_ok=True)
    paths = {u: os.path.join(isa_dir, u + ".s") for u in UNITS}
    cmds = unit_commands(hipcc, "listing", paths.get, extra)
    run_parallel([cmds[u] for u in UNITS if not (reuse and os.path.exists(paths[u]))])
    return paths


def build_commands(hipcc, lib_path, extra=()):
    _, objs = _objects(lib_path)
    cmds = list(unit_commands(hipcc, "object", objs.get, extra).values())
    cmds.append([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", *objs.values(), "-o", lib_path])
    return cmds


def compile_and_link(hipcc, lib_path, extra=()):
    """The units in parallel, then the link; raises LftError with the compiler output on failure."""
    d, _ = _objects(lib_path)
    os.makedirs(d, exist_ok=True)
    cmds = build_commands(hipcc, lib_path, extra)
    run_parallel(cmds[:-1])
    r = subprocess.run(cmds[-1], capture_output=True, text=True)
    if r.returncode != 0:
        raise LftError("link failed:\n" + r.stdout + r.stderr)


class GuardSegment(ctypes.Structure):          # lft_segment
    _fields_ = [("first", c_longlong), ("count", c_longlong), ("trainable", c_int)]


class GuardReport(ctypes.Structure):           # lft_guard_report
    _fields_ = [("grad_norm", c_float), ("clip_coef", c_float), ("skipped_last", c_int), ("bad_segment", c_int),
                ("nonfinite_last", c_longlong), ("steps_applied", c_longlong), ("steps_skipped", c_longlong),
                ("steps_clipped", c_longlong), ("seg_norm", c_float * GUARD_MAX_SEGMENTS)]


def _ctype(ctype: str, where: str):
    """ctypes type of a C type as the headers write it: scalars exactly, const char* and size_t* typed, every other pointer and
    the callback typedef lft_bucket_fn as c_void_p.  A scalar this does not know is an error, not a guess."""
    base = " ".join(re.sub(r"\bconst\b|\*", " ", ctype).split())
    if "*" in ctype:
        return {"const char*": c_char_p, "size_t*": POINTER(c_size_t)}.get(ctype.strip(), c_void_p)
    if base == "lft_bucket_fn":
        return c_void_p
    if base not in _SCALARS:
        raise LftError(f"{where}: no ctypes type for the C type '{ctype.strip()}'")
    return _SCALARS[base]


def _prototypes(header: str) -> dict:
    """{name: (restype, [argtypes], the last parameter's name)} of every `int lft_...(...);` and `const char* lft_...(...);` of a
    header (one parameter = type + name, or `void` for none)."""
    sigs = {}
    for res, name, params in re.findall(r"^(int|const char\*)\s+(lft_\w+)\s*\(([^)]*)\)\s*;", _header_text(header), flags=re.M):
        args = [] if params.strip() == "void" else [re.match(r"(.*?)(\w+)\s*$", p, flags=re.S).groups() for p in params.split(",")]
        sigs[name] = (_ctype(res, name), [_ctype(a, name) for a, _ in args], args[-1][1] if args else None)
    return sigs


_SCALARS = {"int": c_int, "unsigned": ctypes.c_uint, "float": c_float, "double": ctypes.c_double, "long long": c_longlong, "size_t": c_size_t}
TEST_EXPORTS = tuple(_prototypes("lft_hip_test.h"))             # declared in include/lft_hip_test.h, not in the product header
_PROTOTYPES = {**_prototypes("lft_hip.h"), **_prototypes("lft_hip_test.h")}
_SIGS = {name: (res, args) for name, (res, args, _) in _PROTOTYPES.items()}
# the entry points enqueue() serves: the last declared parameter is `void* stream`
STREAM_LAST = frozenset(name for name, (_, args, last) in _PROTOTYPES.items() if last == "stream" and args[-1] is c_void_p)
EXPORTS = tuple(_SIGS)
GUARD_EXPORTS = ("lft_guard_bytes", "lft_guard_init", "lft_adam_step_guarded", "lft_guard_read")   # added to ABI 5 without a new version number
EMA_EXPORTS = ("lft_ema_update",)                                                                  # likewise
LOSS_EXPORTS = ("lft_lf_loss_scratch_bytes", "lft_lf_loss")                                         # likewise
SSIM_LOSS_EXPORTS = ("lft_ssim_loss_scratch_bytes", "lft_ssim_loss")                                 # likewise
REFOCUS_EXPORTS = ("lft_refocus",)                                                                   # likewise
DISPARITY_EXPORTS = ("lft_disparity_scratch_bytes", "lft_disparity")                                 # likewise
# View synthesis, semi-global aggregation, the visibility test, the occlusion-aware sweep, the subset's all-in-focus image, the sheared scene tiling, the blended integrate, the angular tiling of a field, the refinement of a disparity map and the focal-stack term are declared in headers of their own (ADDON_HEADERS) and bound from a table of their
# own: _SIGS, EXPORTS, STREAM_LAST and TEST_EXPORTS are the two older headers' and keep their contents.
_ADDON_PROTOTYPES = {h: _prototypes(h) for h in ADDON_HEADERS}
_ADDON_SIGS = {name: (res, args) for protos in _ADDON_PROTOTYPES.values() for name, (res, args, _) in protos.items()}
ADDON_STREAM_LAST = frozenset(name for protos in _ADDON_PROTOTYPES.values() for name, (_, args, last) in protos.items()
                              if last == "stream" and args[-1] is c_void_p)
VIEW_EXPORTS = tuple(_ADDON_PROTOTYPES["lft_hip_views.h"])                                          # lft_view_render_scratch_bytes, lft_view_render
VIEW_STREAM_LAST = ADDON_STREAM_LAST & frozenset(VIEW_EXPORTS)
SGM_EXPORTS = tuple(_ADDON_PROTOTYPES["lft_hip_sgm.h"])                                             # lft_sgm_scratch_bytes, lft_sgm
VISIBILITY_EXPORTS = tuple(_ADDON_PROTOTYPES["lft_hip_visibility.h"])   # lft_view_visible_scratch_bytes, lft_view_warp_disparity, lft_view_render_visible
OCCLUSION_EXPORTS = tuple(_ADDON_PROTOTYPES["lft_hip_occlusion.h"])     # lft_disparity_occ_scratch_bytes, lft_disparity_occ, lft_occ_gather
AIF_EXPORTS = tuple(_ADDON_PROTOTYPES["lft_hip_aif.h"])                 # lft_aif_at
SHEAR_EXPORTS = tuple(_ADDON_PROTOTYPES["lft_hip_shear.h"])             # lft_scene_divide_shear, lft_scene_integrate_shear, lft_shear_vote
BLEND_EXPORTS = tuple(_ADDON_PROTOTYPES["lft_hip_blend.h"])             # lft_scene_integrate_blend
FIELD_EXPORTS = tuple(_ADDON_PROTOTYPES["lft_hip_field.h"])             # lft_field_counts, lft_field_divide, lft_field_integrate
REFINE_EXPORTS = tuple(_ADDON_PROTOTYPES["lft_hip_refine.h"])           # lft_disp_check, lft_disp_fill, lft_disp_wmedian
FOCAL_EXPORTS = tuple(_ADDON_PROTOTYPES["lft_hip_focal.h"])             # lft_focal_loss_scratch_bytes, lft_focal_loss, lft_refocus_adjoint
# what an older LFT_LIB_PATH build of the same ABI version (A/B runs) may lack: lib() binds everything else unconditionally
OPTIONAL_EXPORTS = frozenset(TEST_EXPORTS + GUARD_EXPORTS + EMA_EXPORTS + LOSS_EXPORTS + SSIM_LOSS_EXPORTS + REFOCUS_EXPORTS + DISPARITY_EXPORTS + VIEW_EXPORTS
                             + SGM_EXPORTS + VISIBILITY_EXPORTS + OCCLUSION_EXPORTS + AIF_EXPORTS + SHEAR_EXPORTS + BLEND_EXPORTS + FIELD_EXPORTS + REFINE_EXPORTS + FOCAL_EXPORTS)
BUCKET_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_int, c_size_t, c_size_t)     # lft_bucket_fn of include/lft_hip.h: 0 = go on, else stop


def lib() -> ctypes.CDLL:
    """Load (once) the in-tree shared library; raise loudly if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LftError(f"{LIB_PATH} is missing: the HIP extension has not been built "
                           "(run __graft_entry__.build()); there is no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        L.lft_version.restype, L.lft_version.argtypes = c_int, []
        got = L.lft_version()
        if got != ABI_VERSION:              # a stale or foreign LFT_LIB_PATH build: its entry points may take other arguments
            raise LftError(f"{LIB_PATH} reports ABI version {got}, this binding needs {ABI_VERSION}: rebuild it (__graft_entry__.build())")
        for name, (res, args) in {**_SIGS, **_ADDON_SIGS}.items():
            if name in OPTIONAL_EXPORTS and not hasattr(L, name):
                continue        # everything else is there, and asking the library for a missing entry point raises
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().lft_last_error()
        raise LftError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def call(name: str, *args) -> None:
    """The entry point `name` with `args`; a non-zero status raises LftError with the library's message."""
    check(getattr(lib(), name)(*args), name)


def query(name: str, *args):
    """A size query: `args` without the trailing `size_t*` parameters of `name`, which come back as an int (several: a tuple)."""
    types = {**_SIGS, **_ADDON_SIGS}.get(name, (None, []))[1]
    outs = [c_size_t(0) for t in types if t is POINTER(c_size_t)]
    if not outs or types[-len(outs):] != [POINTER(c_size_t)] * len(outs):
        raise LftError(f"{name} is no size query: its prototype does not end in a size_t* parameter")
    call(name, *args, *[ctypes.byref(o) for o in outs])
    return outs[0].value if len(outs) == 1 else tuple(o.value for o in outs)


def stream_ptr(device) -> int:
    """The handle of the current stream of `device` (a torch device), as the `void* stream` of an entry point."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def enqueue(name: str, device, *args) -> None:
    """call(name, *args, stream_ptr(device)) with `device` current, for an entry point whose last parameter is `void* stream`."""
    if name not in STREAM_LAST and name not in ADDON_STREAM_LAST:
        raise LftError(f"{name} does not take its stream last: use call() with stream_ptr(device)")
    import torch
    with torch.cuda.device(device):
        call(name, *args, stream_ptr(device))


def ptr_array(tensors):
    return (c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def strides_array(t):
    """The element strides of a tensor, or the numbers of a sequence, as a C array of long long."""
    strides = t.stride() if hasattr(t, "stride") else t
    return (c_longlong * len(strides))(*strides)


def packed_bytes(A, h, w, s, prec) -> int:
    return query("lft_packed_bytes", A, h, w, s, prec)


def workspace_bytes(B, A, h, w, s, prec) -> int:
    return query("lft_workspace_bytes", B, A, h, w, s, prec)
