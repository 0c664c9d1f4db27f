"""Loader and builder for the gfx950 C-ABI library (include/ude_rk4.h).

The library is built in-tree with hipcc (``build_prebuilt``), one object per
model configuration of ``configs.PREBUILT`` compiled in parallel and linked
into ``_build/libude_rk4.so``.  A configuration that is not prebuilt is
compiled on first use into ``_build/jit/libude_rk4_<key>.so`` (same C-ABI,
one registry entry; ``jit_prebuild`` compiles several ahead of use, side by
side); one the kernels cannot hold is refused there with the reason.  There is no fallback: if no library for a model can be
loaded, the fused solver raises.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import re
import shutil
import subprocess
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

from . import configs as _cfgs

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO_DIR = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
INCLUDE = os.path.join(REPO_DIR, "include")
BUILD = os.path.join(PKG_DIR, "_build")
PREBUILT_LIB = os.path.join(BUILD, "libude_rk4.so")
JIT_DIR = os.path.join(BUILD, "jit")
ARCH = os.environ.get("UDE_OFFLOAD_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
HIP_FLAGS = ["-O3", "-std=c++20", "-fPIC", "-ffp-contract=off", f"--offload-arch={ARCH}"]

UDE_OK, UDE_E_UNSUPPORTED, UDE_E_INVALID, UDE_E_HIP, UDE_E_SOLVER = 0, -1, -2, -3, -4
_ERRS = {UDE_E_UNSUPPORTED: "unsupported model configuration", UDE_E_INVALID: "invalid argument",
         UDE_E_HIP: "HIP runtime error", UDE_E_SOLVER: "adaptive solve failed"}

SUMSQ_WS = 1025          # doubles of ude_scaled_sumsq's output / workspace (UDE_SUMSQ_WS)


class UdeModelDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("n_regions", ctypes.c_int32), ("latent_dim", ctypes.c_int32),
                ("n_p_hidden", ctypes.c_int32), ("p_hidden", ctypes.c_int32 * 4),
                ("n_a_hidden", ctypes.c_int32), ("a_hidden", ctypes.c_int32 * 4)]


class UdeProblem(ctypes.Structure):
    _fields_ = [("n_traj", ctypes.c_int32), ("n_steps", ctypes.c_int32), ("n_out", ctypes.c_int32),
                ("fa_w", ctypes.c_float), ("recompute", ctypes.c_int32)]


class UdeDopriInfo(ctypes.Structure):
    _fields_ = [("n_steps", ctypes.c_int32), ("n_accepted", ctypes.c_int32), ("n_evals", ctypes.c_int32),
                ("status", ctypes.c_int32)]


class UdeSizes(ctypes.Structure):
    _fields_ = [("pack_bytes", ctypes.c_int64), ("sched_bytes", ctypes.c_int64), ("ckpt_bytes", ctypes.c_int64),
                ("stats_slab_bytes", ctypes.c_int64), ("grad_slab_bytes", ctypes.c_int64),
                ("n_params", ctypes.c_int64), ("grid_fwd", ctypes.c_int32), ("grid_bwd", ctypes.c_int32),
                ("lds_fwd", ctypes.c_int32), ("lds_bwd", ctypes.c_int32),
                ("dec_pack_bytes", ctypes.c_int64), ("ckpt_final_bytes", ctypes.c_int64),
                ("dec_ws_bytes", ctypes.c_int64), ("act_bytes", ctypes.c_int64), ("ctl_bytes", ctypes.c_int64)]


class UdeSideStats(ctypes.Structure):
    """mean (2) / std (2) / fa_norm (1) float buffers and the fp64 totals (5, nullable)."""
    _fields_ = [("mean", ctypes.c_void_p), ("std", ctypes.c_void_p), ("fa_norm", ctypes.c_void_p),
                ("sums", ctypes.c_void_p)]


class UdeSideStatsGrad(ctypes.Structure):
    """Cotangents of mean / std / fa_norm (each nullable: zero)."""
    _fields_ = [("d_mean", ctypes.c_void_p), ("d_std", ctypes.c_void_p), ("d_fa_norm", ctypes.c_void_p)]


def make_desc(cfg: _cfgs.Config) -> UdeModelDesc:
    kind, R, L, net, aug = cfg
    d = UdeModelDesc()
    d.kind = _cfgs.KIND_CODE[kind]
    d.n_regions = R
    d.latent_dim = L
    net = list(net or [])
    aug = list(aug or [])
    d.n_p_hidden = len(net)
    d.n_a_hidden = len(aug)
    for i, v in enumerate(net):
        d.p_hidden[i] = v
    for i, v in enumerate(aug):
        d.a_hidden[i] = v
    return d


class UdeError(RuntimeError):
    pass


class UdeStaleLibrary(UdeError):
    """The prebuilt library does not match the sources in the tree."""


def check(rc: int, what: str) -> None:
    if rc != UDE_OK:
        raise UdeError(f"{what} failed: {_ERRS.get(rc, rc)} (code {rc})")


_vp, _i32, _i64, _f32, _f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double
_pd, _pp, _pvp, _pi64 = ctypes.POINTER(UdeModelDesc), ctypes.POINTER(UdeProblem), ctypes.POINTER(_vp), ctypes.POINTER(_i64)
_pst, _pdst = ctypes.POINTER(UdeSideStats), ctypes.POINTER(UdeSideStatsGrad)


def _sig(method: Optional[str], *groups) -> tuple:
    """(NativeLib method generated for the function or None, its argument types); a group is one type or
    (count, type)."""
    types: List[object] = []
    for g in groups:
        types += [g[1]] * g[0] if isinstance(g, tuple) else [g]
    return method, tuple(types)


# The binding's one table: every function of include/ude_rk4.h -> its argument types, in the header's
# order.  Each returns int (an UDE_E_* code) except ude_build_info.  A function with a method name gets
# the method NativeLib.<name>(*args) = check(function(*args)); the others have a hand-written method that
# does more.  A ctypes Structure (or c_int64) passed where the table says POINTER(T) goes by reference.
_CABI: Dict[str, tuple] = {
    "ude_supported": _sig(None, _pd),
    "ude_query": _sig(None, _pd, _pp, _i32, ctypes.POINTER(UdeSizes)),
    "ude_pack_weights": _sig(None, _pd, _pvp, _pvp, (2, _vp)),
    "ude_pack_weights_bayes": _sig(None, _pd, _pp, (4, _pvp), (3, _vp)),
    "ude_rk4_forward": _sig("forward", _pd, _pp, (8, _vp)),
    "ude_rk4_backward": _sig("backward", _pd, _pp, (11, _vp)),
    "ude_rk4_backward_sir": _sig("backward_sir", _pd, _pp, (12, _vp)),
    "ude_rk4_forward_ex": _sig("forward_ex", _pd, _pp, (7, _vp), _pst, _vp),
    "ude_rk4_forward_dec_ex": _sig("forward_dec_ex", _pd, _pp, (9, _vp), _pst, (2, _vp)),
    "ude_rk4_backward_ex": _sig("backward_ex", _pd, _pp, (6, _vp), _pst, _pdst, (5, _vp)),
    "ude_dopri5_workspace": _sig(None, _pd, _pp, _i32, _pi64),
    "ude_dopri5_forward": _sig(None, _pd, _pp, (2, _vp), (3, _f64), _i32, (4, _vp), ctypes.POINTER(UdeDopriInfo), _vp),
    "ude_loss_head_workspace": _sig(None, _pd, (4, _i32), _pi64),
    "ude_loss_head_forward": _sig("loss_forward", _pd, (3, _i32), (7, _vp)),
    "ude_loss_head_backward": _sig("loss_backward", _pd, (3, _i32), (10, _vp)),
    "ude_loss_head_backward_sir": _sig("loss_backward_sir", _pd, (3, _i32), (10, _vp)),
    "ude_rhs_workspace": _sig(None, _pd, _pp, _i32, _pi64),
    "ude_rhs_forward": _sig("rhs_forward", _pd, _pp, (6, _vp)),
    "ude_rhs_vjp": _sig("rhs_vjp", _pd, _pp, (9, _vp)),
    "ude_pack_decoder": _sig("pack_decoder", _pd, (4, _vp)),
    "ude_rk4_forward_dec": _sig("forward_dec", _pd, _pp, (11, _vp)),
    "ude_decoder_backward": _sig("decoder_backward", _pd, _pp, (10, _vp)),
    "ude_nll_workspace": _sig(None, _pd, (3, _i32), _pi64),
    "ude_nll_forward": _sig("nll_forward", _pd, (3, _i32), (5, _vp)),
    "ude_nll_backward": _sig("nll_backward", _pd, (3, _i32), (6, _vp)),
    "ude_crps_workspace": _sig(None, (4, _i32), _pi64),
    "ude_crps_forward": _sig("crps_forward", (5, _i32), (5, _vp)),
    "ude_crps_backward": _sig("crps_backward", (5, _i32), (4, _vp)),
    "ude_energy_workspace": _sig(None, (5, _i32), _pi64),
    "ude_energy_forward": _sig("energy_forward", (6, _i32), (5, _vp)),
    "ude_energy_backward": _sig("energy_backward", (6, _i32), (5, _vp)),
    "ude_rhs_eval_vjp": _sig("rhs_eval_vjp", _pd, _pp, (4, _vp), _f32, (4, _vp)),
    "ude_lincomb": _sig(None, _i64, _vp, _pvp, _i32, (3, _vp)),
    "ude_scaled_sumsq": _sig("scaled_sumsq", _i64, (3, _vp), (2, _f64), (2, _vp)),
    "ude_lincomb_hc": _sig(None, _i64, _vp, _pvp, _i32, ctypes.POINTER(_f32), (2, _vp)),
    "ude_dopri_ratio": _sig(None, (3, _vp), (2, _f64), _vp, _pi64, _i32, _vp, _i32, _f64, (3, _vp)),
    "ude_rk4_forecast_dec": _sig("forecast_dec", _pd, _pp, (7, _vp), _pst, _vp),
    "ude_rk4_forecast_dyn": _sig("forecast_dyn", _pd, _pp, (8, _vp), _pst, _vp),
    "ude_rk4_forecast_scn": _sig("forecast_scn", _pd, _pp, (9, _vp), _pst, _vp),
    "ude_forecast_summary_workspace": _sig(None, (5, _i32), _pi64),
    "ude_forecast_summary": _sig("forecast_summary", (4, _i32), (4, _vp), _i32, (6, _vp)),
    "ude_forecast_verify_workspace": _sig(None, (7, _i32), _pi64),
    "ude_forecast_verify": _sig("forecast_verify", (4, _i32), (4, _vp), _i32, _vp, (2, _i32), (8, _vp)),
    "ude_forecast_season_workspace": _sig(None, (9, _i32), _pi64),
    "ude_forecast_season": _sig("forecast_season", (8, _i32), (5, _vp), _i32, (8, _vp)),
    "ude_forecast_joint_workspace": _sig(None, (7, _i32), _pi64),
    "ude_forecast_joint": _sig("forecast_joint", (7, _i32), (11, _vp)),
    "ude_forecast_aggregate": _sig("forecast_aggregate", _i64, (2, _i32), (6, _vp)),
    "ude_forecast_aggregate_dyn": _sig("forecast_aggregate_dyn", _i32, _i64, (2, _i32), (5, _vp)),
    "ude_build_info": _sig(None),
}
EXPORTED_SYMBOLS = tuple(_CABI)
# integer / float arguments accept whatever int() / float() accept (numpy and torch scalars)
_CONV = {_i32: int, _i64: int, _f32: float, _f64: float}


def _converting(fn, types):
    """fn with the table's integer / float positions converted; fn itself when there are none.  Resolved once
    per function, so a call costs no more than the ctypes call and its conversions."""
    conv = tuple((i, _CONV[t]) for i, t in enumerate(types) if t in _CONV)
    if not conv:
        return fn

    def call(*args):
        args = list(args)
        for i, c in conv:
            args[i] = c(args[i])
        return fn(*args)
    return call


class NativeLib:
    """ctypes view of one libude_rk4*.so: the methods generated from ``_CABI`` (below the class: forward,
    backward_ex, ...) and the hand-written ones."""

    def __init__(self, path: str):
        self.path = path
        self.lib = ctypes.CDLL(path)
        self._raw = {}
        for cname, (name, types) in _CABI.items():
            fn = getattr(self.lib, cname)
            fn.argtypes = list(types)
            fn.restype = ctypes.c_char_p if cname == "ude_build_info" else ctypes.c_int
            self._raw[cname] = _converting(fn, types)

    def _rc(self, cname: str, *args) -> int:
        return self._raw[cname](*args)

    def _call(self, cname: str, *args) -> None:
        check(self._raw[cname](*args), cname)

    def _workspace(self, cname: str, *args) -> int:
        out = ctypes.c_int64(0)
        self._call(cname, *args, out)
        return int(out.value)

    def supported(self, desc: UdeModelDesc) -> bool:
        return bool(self._rc("ude_supported", desc))

    def query(self, desc, prob, device: int) -> UdeSizes:
        out = UdeSizes()
        self._call("ude_query", desc, prob, device, out)
        return out

    def pack(self, desc, w_ptrs: Sequence[int], b_ptrs: Sequence[int], pack_ptr: int, stream: int) -> None:
        arr = lambda ptrs: (ctypes.c_void_p * len(w_ptrs))(*ptrs)
        self._call("ude_pack_weights", desc, arr(w_ptrs), arr(b_ptrs), pack_ptr, stream)

    def pack_bayes(self, desc, prob, w_mean: Sequence[int], b_mean: Sequence[int], w_std: Sequence[int],
                   b_std: Sequence[int], eps_ptr: int, pack_ptr: int, stream: int) -> None:
        arr = lambda ptrs: (ctypes.c_void_p * len(w_mean))(*ptrs)
        self._call("ude_pack_weights_bayes", desc, prob, arr(w_mean), arr(b_mean), arr(w_std), arr(b_std), eps_ptr,
                   pack_ptr, stream)

    def dopri5_workspace(self, desc, prob, device: int) -> int:
        return self._workspace("ude_dopri5_workspace", desc, prob, device)

    def dopri5_forward(self, desc, prob, pack, t_out, rtol, atol, first_step, max_steps, y0, latent, ws,
                       stats_out, stream) -> UdeDopriInfo:
        info = UdeDopriInfo()
        rc = self._rc("ude_dopri5_forward", desc, prob, pack, t_out, rtol, atol, first_step, max_steps, y0, latent,
                      ws, stats_out, info, stream)
        if rc == UDE_E_SOLVER:
            why = {1: "underflow in dt", 2: "max_num_steps exceeded", 3: "non-finite values in state `y`"}
            raise AssertionError(f"dopri5: {why.get(info.status, info.status)} "
                                 f"(after {info.n_steps} steps, {info.n_evals} evaluations)")
        check(rc, "ude_dopri5_forward")
        return info

    def loss_workspace(self, desc, T, S, B, device) -> int:
        return self._workspace("ude_loss_head_workspace", desc, T, S, B, device)

    def rhs_workspace(self, desc, prob, device: int) -> int:
        return self._workspace("ude_rhs_workspace", desc, prob, device)

    def nll_workspace(self, desc, T, S, B) -> int:
        return self._workspace("ude_nll_workspace", desc, T, S, B)

    def crps_workspace(self, T, S, B, R) -> int:
        return self._workspace("ude_crps_workspace", T, S, B, R)

    def energy_workspace(self, T, S, B, R, block) -> int:
        return self._workspace("ude_energy_workspace", T, S, B, R, block)

    def energy_supported(self, T, S, B, R, block) -> bool:
        """Whether the energy kernels take this shape (the limits live in csrc/ude_energy.h alone)."""
        return self._rc("ude_energy_workspace", T, S, B, R, block, ctypes.c_int64(0)) == UDE_OK

    def forecast_summary_workspace(self, T, S, B, R, n_q) -> int:
        return self._workspace("ude_forecast_summary_workspace", T, S, B, R, n_q)

    def forecast_verify_workspace(self, T, S, B, R, n_q, n_alpha, n_pit) -> int:
        return self._workspace("ude_forecast_verify_workspace", T, S, B, R, n_q, n_alpha, n_pit)

    def forecast_season_workspace(self, T, S, B, R, n_q, start, every, run, window) -> int:
        return self._workspace("ude_forecast_season_workspace", T, S, B, R, n_q, start, every, run, window)

    def forecast_joint_workspace(self, T, S, B, R, start, every, p_code) -> int:
        return self._workspace("ude_forecast_joint_workspace", T, S, B, R, start, every, p_code)

    def lincomb(self, n, base, ks: Sequence[int], coef, out, stream) -> None:
        arr = (ctypes.c_void_p * len(ks))(*ks)
        self._call("ude_lincomb", n, base, arr, len(ks), coef, out, stream)

    def lincomb_hc(self, n, base, ks: Sequence[int], coef: Sequence[float], out, stream) -> None:
        """ude_lincomb with host coefficients (fp32 values, copied into the launch)."""
        arr = (ctypes.c_void_p * len(ks))(*ks)
        cv = (ctypes.c_float * len(coef))(*coef)
        self._call("ude_lincomb_hc", n, base, arr, len(ks), cv, out, stream)

    def dopri_ratio(self, err, y0, y1, atol, rtol, ssq, ns: Sequence[int], extra, n_extra, dt, flag, status,
                    stream) -> None:
        na = (ctypes.c_int64 * max(len(ns), 1))(*ns)
        self._call("ude_dopri_ratio", err, y0, y1, atol, rtol, ssq, na, len(ns), extra, n_extra, dt, flag, status,
                   stream)

    def build_info(self) -> str:
        return self.lib.ude_build_info().decode()


def _method(cname: str, name: str, n_args: int):
    def method(self, *args) -> None:
        if len(args) != n_args:
            raise TypeError(f"{name} takes {n_args} arguments ({len(args)} given)")
        rc = self._raw[cname](*args)
        if rc != UDE_OK:
            check(rc, cname)
    method.__name__ = name
    method.__doc__ = f"check({cname}(*args)): the arguments of include/ude_rk4.h, in its order."
    return method


for _cname, (_name, _types) in _CABI.items():
    if _name:
        setattr(NativeLib, _name, _method(_cname, _name, len(_types)))


# ---------------------------------------------------------------------------
# building
# ---------------------------------------------------------------------------

def _run(cmd: List[str]) -> None:
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        err = UdeError("build command failed:\n" + " ".join(cmd) + "\n" + r.stdout[-8000:])
        err.output = r.stdout              # the whole log: the first error is rarely in its tail
        raise err


_SRC_HASH: Optional[str] = None


def source_hash(fresh: bool = False) -> str:
    """sha1 (16 hex digits) of every source the library is compiled from (csrc/*.h, csrc/*.hip,
    include/ude_rk4.h) and of the compile flags.  Embedded in ``ude_build_info`` so a prebuilt
    library that no longer matches the tree is refused at load (``prebuilt``).  Computed once per
    process (the tree the process started from); ``fresh`` re-reads the sources (the builder)."""
    global _SRC_HASH
    if _SRC_HASH is not None and not fresh:
        return _SRC_HASH
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip")))
    srcs.append(os.path.join(INCLUDE, "ude_rk4.h"))
    h = hashlib.sha1()
    for f in srcs:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(HIP_FLAGS).encode())
    _SRC_HASH = h.hexdigest()[:16]
    return _SRC_HASH


_INFO_HASH = re.compile(r"\bsrc=([0-9a-f]+)")
_INFO_EXTRA = re.compile(r"\bextra_flags=\[(.*)\]")


def _c_string(s: str) -> str:
    return s.replace("\\", "\\\\").replace('"', '\\"')


def build_library(cfgs: Sequence[_cfgs.Config], out_path: str, tag: str, jobs: Optional[int] = None,
                  extra_flags: Sequence[str] = ()) -> str:
    """Compile one object per configuration + the C-ABI, link into out_path."""
    if not os.path.exists(HIPCC):
        raise UdeError(f"hipcc not found ({HIPCC}); cannot build the gfx950 library")
    gen = os.path.join(BUILD, "gen_" + tag)
    os.makedirs(gen, exist_ok=True)
    reg = ["// generated by ude_amd/_native.py -- do not edit", "namespace ude {"]
    reg += [f"extern const Entry ude_entry_{i};" for i in range(len(cfgs))]
    reg.append("const Entry* const kEntries[] = {" + ", ".join(f"&ude_entry_{i}" for i in range(len(cfgs))) + "};")
    reg.append(f"constexpr int kNumEntries = {len(cfgs)};")
    reg.append("}  // namespace ude")
    reg.append(f'#define UDE_REGISTRY_TAG "{tag}:{len(cfgs)}"')
    reg.append(f'#define UDE_SRC_HASH "{source_hash(fresh=True)}"')
    reg.append(f'#define UDE_EXTRA_FLAGS "{_c_string(" ".join(extra_flags))}"')
    with open(os.path.join(gen, "ude_registry.inc"), "w") as f:
        f.write("\n".join(reg) + "\n")
    inc = ["-I", INCLUDE, "-I", CSRC, "-I", gen, *extra_flags]

    def compile_cfg(i_cfg):
        i, cfg = i_cfg
        obj = os.path.join(gen, f"cfg_{i}.o")
        _run([HIPCC, *HIP_FLAGS, *inc, "-c", os.path.join(CSRC, "ude_cfg.hip"), f"-DUDE_CFG_ID={i}",
              f"-DUDE_ONE_CONFIG={_cfgs.template_args(cfg)}", "-o", obj])
        return obj

    jobs = jobs or min(16, os.cpu_count() or 4)
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        objs = list(ex.map(compile_cfg, list(enumerate(cfgs))))
    capi = os.path.join(gen, "ude_rk4.o")
    _run([HIPCC, *HIP_FLAGS, *inc, "-c", os.path.join(CSRC, "ude_rk4.hip"), "-o", capi])
    tmp = out_path + ".tmp"
    _run([HIPCC, *HIP_FLAGS, "-shared", *objs, capi, "-o", tmp])
    os.replace(tmp, out_path)
    return out_path


def build_prebuilt(jobs: Optional[int] = None) -> str:
    os.makedirs(BUILD, exist_ok=True)
    return build_library(_cfgs.PREBUILT, PREBUILT_LIB, "prebuilt", jobs)


# ---------------------------------------------------------------------------
# loading
# ---------------------------------------------------------------------------

_lock = threading.Lock()
_loaded: Dict[str, NativeLib] = {}


def _load(path: str) -> NativeLib:
    with _lock:
        if path not in _loaded:
            _loaded[path] = NativeLib(path)
        return _loaded[path]


def built_hash(lib: NativeLib) -> Optional[str]:
    m = _INFO_HASH.search(lib.build_info())
    return m.group(1) if m else None


_verified: Dict[str, bool] = {}


def prebuilt() -> NativeLib:
    """The in-tree prebuilt library; refused if it was built from other sources than the tree's
    (a stale binary would silently run old kernels) or with extra compile flags (an A/B or
    diagnostic build -- -DUDE_ABL, -DUDE_PROFILE -- placed at the product path).  Checked once per
    process: the library a process has loaded does not change when the sources are edited."""
    if not os.path.exists(PREBUILT_LIB):
        raise UdeError(f"{PREBUILT_LIB} is missing: run __graft_entry__.build() (hipcc, gfx950)")
    lib = _load(PREBUILT_LIB)
    if not _verified.get(PREBUILT_LIB):
        got, want = built_hash(lib), source_hash()
        if got != want:
            raise UdeStaleLibrary(f"{PREBUILT_LIB} is stale (built from sources {got}, tree is {want}): "
                                  "rebuild it with __graft_entry__.build()")
        m = _INFO_EXTRA.search(lib.build_info())
        if m is None or m.group(1).strip():
            raise UdeStaleLibrary(f"{PREBUILT_LIB} was built with extra flags [{m.group(1) if m else '?'}] "
                                  "(a development build): rebuild it with __graft_entry__.build()")
        _verified[PREBUILT_LIB] = True
    return lib


def jit_path(cfg: _cfgs.Config) -> str:
    return os.path.join(JIT_DIR, f"libude_rk4_{_cfgs.config_key(cfg)}_{source_hash()[:10]}.so")


_STATIC_ASSERT = re.compile(r"static assertion failed[^\n]*")


def _jit_build(cfg: _cfgs.Config) -> str:
    path = jit_path(cfg)
    if not os.path.exists(path):
        os.makedirs(JIT_DIR, exist_ok=True)
        try:
            build_library([cfg], path, f"jit_{_cfgs.config_key(cfg)}_{source_hash()[:10]}", jobs=1)
        except UdeError as e:
            # a configuration the kernels cannot hold (csrc/ude_model.h's static_asserts: the record does not
            # fit the LDS, ...) is refused here, with the compiler's reason, never at launch
            why = sorted(set(_STATIC_ASSERT.findall(getattr(e, "output", str(e)))))
            if why:
                raise UdeError(f"unsupported model configuration {cfg}: " + "; ".join(why)) from e
            raise
    return path


def jit_library(cfg: _cfgs.Config) -> NativeLib:
    return _load(_jit_build(cfg))


def jit_prebuild(cfgs: Sequence[_cfgs.Config], jobs: Optional[int] = None) -> List[str]:
    """Build the missing JIT libraries of several configurations in parallel (at most 16 compiles at a time),
    each at the path ``jit_library`` uses, so ``library_for`` finds them as after a first use.  Configurations
    of ``configs.PREBUILT`` are skipped.  Returns the libraries' paths; raises the first build's ``UdeError``
    after every build has ended."""
    todo = [c for c in dict.fromkeys(cfgs) if c not in _cfgs.PREBUILT]
    jobs = max(1, min(16, jobs or os.cpu_count() or 4, len(todo) or 1))
    source_hash()                                   # read the sources once, before the threads ask
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        futs = [ex.submit(_jit_build, c) for c in todo]
    errs = [f.exception() for f in futs if f.exception() is not None]
    if errs:
        raise errs[0]
    return [f.result() for f in futs]


def library_for(cfg: _cfgs.Config) -> NativeLib:
    """The library that has a kernel for this configuration (JIT-compiling if needed)."""
    desc = make_desc(cfg)
    if os.path.exists(PREBUILT_LIB):
        lib = prebuilt()
        if lib.supported(desc):
            return lib
    lib = jit_library(cfg)
    if not lib.supported(desc):
        raise UdeError(f"no gfx950 kernel for {cfg}")
    return lib


_SUPPORTED: Dict[_cfgs.Config, bool] = {}


def config_supported(cfg: _cfgs.Config) -> bool:
    """Whether a fused kernel exists (prebuilt, or JIT-compiled here) for cfg.

    Bayesian models keep a second dW accumulator per tile in registers; models
    too large for that are compiled but report unsupported (Model::FITS)."""
    hit = _SUPPORTED.get(cfg)
    if hit is None:
        try:
            library_for(cfg)
            hit = True
        except UdeStaleLibrary:
            raise
        except UdeError:
            hit = False
        _SUPPORTED[cfg] = hit
    return hit


def loaded_paths() -> List[str]:
    return sorted(_loaded)
