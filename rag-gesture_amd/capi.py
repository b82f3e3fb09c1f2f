"""ctypes binding of the C-ABI HIP extension (include/rg_gesture.h).

The product path has no CPU or PyTorch fallback: if librg_gesture.so is missing or fails
to load, or no GPU is present, every op raises.

The header is the only place an argument block or an RG_* constant is declared: `struct(name)` and `header_constants()`
derive the ctypes classes and values from it, and every launch goes through `Handle.call`, which checks its arguments
against the header's prototype.
"""
import contextlib
import ctypes
import functools
import gc
import os
import re

import torch

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_TAG = "diag" if os.environ.get("RG_DIAG") == "1" else os.environ.get("RG_LIB_TAG", "")    # (see build.py: diagnostic / experiment builds)
LIB_PATH = os.path.join(PKG_DIR, "librg_gesture%s.so" % ("_" + _TAG if _TAG else ""))
HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "rg_gesture.h")

_lib = None


class RgError(RuntimeError):
    pass


class RgConfigError(RgError, AssertionError):
    """An argument / configuration check that the reference states as an `assert` (e.g. the inference_kwargs compatibility
    rules, diffusion_architecture.py:227-241): still an AssertionError for callers that catch one, but raised explicitly,
    so it does not disappear under `python -O`."""


def require(cond, msg="unsupported configuration"):
    if not cond:
        raise RgConfigError(msg)


@functools.lru_cache(None)
def _header_text():
    """include/rg_gesture.h without its comments."""
    with open(HEADER_PATH) as f:
        text = f.read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_symbols():
    """Every entry point include/rg_gesture.h declares."""
    return sorted(set(re.findall(r"\b(rg_[a-z0-9_]+)\s*\(", _header_text())))


def header_version():
    """RG_VERSION of include/rg_gesture.h."""
    v = header_constants().get("RG_VERSION")
    if v is None:
        raise RgError("include/rg_gesture.h defines no RG_VERSION")
    return v


_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "int64_t": ctypes.c_int64,
            "long long": ctypes.c_longlong, "unsigned char": ctypes.c_ubyte,
            "float": ctypes.c_float, "double": ctypes.c_double}
_STRUCT_RE = r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;"


def _parse_constants(text):
    """name -> int for the `#define RG_* <integer expression>` lines of a comment-free header text; defines without a value
    (the include guard) or with another kind of value are skipped."""
    consts = {}
    for name, expr in re.findall(r"^#define[ \t]+(RG_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        expr = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]+\b", r"\1", expr)          # integer suffixes
        if re.fullmatch(r"(0[xX][0-9a-fA-F]+|\d+|[\s()<>+\-*|&])+", expr):
            consts[name] = int(eval(expr, {"__builtins__": {}}))
    return consts


def _parse_structs(text, consts):
    """typedef name -> ctypes.Structure subclass for the `typedef struct ... { ... } name;` blocks of a comment-free header
    text.  Members: pointers (void*), _SCALARS, earlier structs by value, fixed arrays of either sized by a literal or a
    constant; several declarators per line."""
    structs = {}
    for body, name in re.findall(_STRUCT_RE, text, flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = re.sub(r"\s*([\[\],*])\s*", r"\1", " ".join(decl.split()))
            ptr = re.fullmatch(r"[\w *]*\*(\w+)", decl)
            m = re.fullmatch(r"(?:const )?([\w ]+) ([\w\[\],]+)", decl)
            base = m and (_SCALARS.get(m.group(1)) or structs.get(m.group(1)))
            if ptr:
                fields.append((ptr.group(1), ctypes.c_void_p))
            elif base:
                for d in m.group(2).split(","):
                    d = re.fullmatch(r"(\w+)(?:\[(\d+|RG_\w+)\])?", d)
                    n = d and d.group(2) and (int(d.group(2)) if d.group(2).isdigit() else consts.get(d.group(2)))
                    if not d or (d.group(2) and not n):
                        raise RgError("include/rg_gesture.h: cannot bind member %r of %s" % (decl, name))
                    fields.append((d.group(1), base * n if n else base))
            elif decl:
                raise RgError("include/rg_gesture.h: cannot bind member %r of %s" % (decl, name))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": "include/rg_gesture.h: %s." % name})
    return structs


@functools.lru_cache(None)
def header_constants():
    """name -> value of every integer `#define RG_*` of include/rg_gesture.h (RG_VERSION, array sizes, mode codes)."""
    return _parse_constants(_header_text())


@functools.lru_cache(None)
def header_structs():
    """typedef name -> ctypes.Structure subclass for every argument block include/rg_gesture.h declares."""
    return _parse_structs(_header_text(), header_constants())


def struct(name):
    """The ctypes class of the header's argument block `name` (e.g. "rg_seq_args")."""
    if name not in header_structs():
        raise RgError("include/rg_gesture.h declares no argument block %s" % name)
    return header_structs()[name]


def header_prototypes():
    """name -> (restype, [argtypes]) for every function include/rg_gesture.h declares: pointers (device or host) are
    void*, scalars keep their C width, so ctypes converts and range-checks every argument instead of guessing."""
    text = re.sub(_STRUCT_RE, "", _header_text(), flags=re.S)   # struct bodies hold no prototypes
    protos = {}
    for ret, name, args in re.findall(r"\b(int|void|const\s+char\s*\*)\s+(rg_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        argtypes = []
        args = " ".join(args.split())
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    argtypes.append(ctypes.c_void_p)
                    continue
                ty = " ".join(a.replace("const ", "").split()[:-1])
                if ty not in _SCALARS:
                    raise RgError("include/rg_gesture.h: cannot bind argument %r of %s" % (a, name))
                argtypes.append(_SCALARS[ty])
        restype = None if ret == "void" else (ctypes.c_char_p if "char" in ret else ctypes.c_int)
        protos[name] = (restype, argtypes)
    return protos


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RgError("HIP extension not built: %s is missing (run __graft_entry__.build())" % LIB_PATH)
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.rg_version.restype = ctypes.c_int
        want, got = header_version(), _lib.rg_version()
        if want != got:      # (argument blocks are passed by pointer: a library built against another header would misread them silently)
            _lib = None
            raise RgError("%s is ABI version %d, include/rg_gesture.h is %d: rebuild (__graft_entry__.build())" % (LIB_PATH, got, want))
        for name, (restype, argtypes) in header_prototypes().items():
            fn = getattr(_lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _lib.rg_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    return _lib


def _convert(a):
    """Tensors -> device pointers; everything else is converted (and range-checked) by the prototype's argtypes."""
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise RgError("device tensor expected, got a CPU tensor")
        if not a.is_contiguous():
            raise RgError("contiguous tensor expected")
        return a.data_ptr()
    if isinstance(a, bool):
        return int(a)
    return a


class I64(int):
    """Kept for callers that mark int64_t arguments; the width now comes from the header's prototype."""


class Handle:
    """One rg_handle per device; calls on a handle are serialised by the caller."""

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise RgError("no GPU visible: the HIP path cannot run (there is no CPU fallback)")
        lib = load_library()
        self.lib = lib
        self.device = torch.cuda.current_device() if device is None else int(device)
        h = ctypes.c_void_p()
        rc = lib.rg_create(ctypes.byref(h), self.device)
        if rc != 0:
            raise RgError("rg_create failed with %d" % rc)
        self._h = h
        self.recorder = None      # an OpRecorder while launches are being recorded instead of issued (vae.py)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.rg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def call(self, name, *args, stream=None, keep=None):
        """Invoke rg_<name>(handle, *args, stream) and raise on a non-zero status.  keep: objects (argument blocks, tensors an
        argument block points into) that must stay alive until the launch has been issued (recording)."""
        if self.recorder is not None and stream is None:
            self.recorder.add((name, args, keep))   # (the tensors in args / keep stay alive until the recorder has issued)
            return
        fn = getattr(self.lib, "rg_" + name)
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        if fn.argtypes is None or len(fn.argtypes) != len(args) + 2:
            raise RgError("rg_%s takes %s arguments besides handle and stream, got %d"
                          % (name, "?" if fn.argtypes is None else len(fn.argtypes) - 2, len(args)))
        try:
            rc = fn(self._h, *[_convert(a) for a in args], s)
        except ctypes.ArgumentError as e:
            raise RgError("rg_%s: %s" % (name, e))
        if rc != 0:
            raise RgError("rg_%s failed (%d): %s" % (name, rc, self.lib.rg_last_error(self._h).decode()))


@contextlib.contextmanager
def capture(graph):
    """torch.cuda.graph(graph) with Python's cyclic garbage collector off: a collection that starts in the middle of a
    capture can finalise objects that own device resources (graphs, events, streams of an earlier model), and a HIP call
    from a finaliser aborts a capturing process.  torch's context collects once before the capture begins."""
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if was:
            gc.enable()


class OpRecorder:
    """Launch sequences of up to 4 independent, structurally identical jobs (the four body-part VAEs: same layers,
    different weights and rows), recorded job by job as the (name, args, keep) of Handle.call and issued position by
    position: where the jobs' i-th launches are the same operation on the same shapes they go out as ONE grouped launch
    (rg_gemm_grouped, rg_layernorm_grouped, ...), otherwise one by one in job order.  Control flow never depends on device
    data, so recording is exact; recorded arguments keep their tensors alive until `issue` (the allocator must not reuse a
    block of job 0 for job 1 while job 0's later launches, issued later, still need it)."""
    # ops whose only argument is a host argument block: rg_<name>_grouped(blocks[n] by value, n)
    BLOCKS = ("gemm", "venc_forward", "vdec_step")
    # name -> positions of the per-job pointer arguments: rg_<name>_grouped(n, ...) takes host arrays of n pointers there and
    # every other argument, which must be equal across the jobs, where rg_<name> has it
    GROUPED = {"layernorm": (0, 1, 2, 3, 6), "add_rows": (0, 1, 2), "copy_rows": (0, 1), "mha_bf16": (0, 2, 4, 6)}

    def __init__(self):
        self.jobs, self.cur = [], None

    def begin_job(self):
        self.cur = []
        self.jobs.append(self.cur)

    def add(self, op):
        self.cur.append(op)

    def _grouped(self, ops):
        """(entry point, args) of the one launch that does the jobs' `ops` of one position, or None."""
        n, (name, a0, _) = len(ops), ops[0]
        if n < 2 or any(op[0] != name for op in ops):
            return None
        if name in self.BLOCKS:
            blocks = [op[1][0]._obj for op in ops]
            return name + "_grouped", (ctypes.byref((type(blocks[0]) * n)(*blocks)), n)
        pidx = self.GROUPED.get(name, ())
        # per job: the shared arguments and which of its pointers are null
        if not pidx or len({tuple(a is None if i in pidx else a for i, a in enumerate(op[1])) for op in ops}) != 1:
            return None
        return name + "_grouped", (n, *[(ctypes.c_void_p * n)(*[_convert(op[1][i]) for op in ops]) if i in pidx else a
                                        for i, a in enumerate(a0)])

    def issue(self, h):
        """Launch everything that was recorded (on the current stream) and forget it."""
        jobs, self.jobs, self.cur = self.jobs, [], None
        s = torch.cuda.current_stream().cuda_stream
        zipped = len(jobs) <= 4 and len({len(j) for j in jobs}) == 1
        for ops in zip(*jobs) if zipped else [(op,) for j in jobs for op in j]:
            g = self._grouped(ops)
            for name, args in [g] if g else [op[:2] for op in ops]:
                h.call(name, *args, stream=s)


_handles = {}


def get_handle(device=None):
    d = torch.cuda.current_device() if device is None else int(device)
    if d not in _handles:
        _handles[d] = Handle(d)
    return _handles[d]


def device_or_fail(device, what):
    """The cuda device `device` names (None: the current one), or an RgError that says `what` cannot run without a GPU."""
    if not torch.cuda.is_available():
        raise RgError("no GPU visible: %s runs on the device (there is no CPU fallback)" % what)
    return torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
