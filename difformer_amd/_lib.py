"""ctypes binding of libdifformer_hip.so (C ABI: include/difformer_hip.h).

There is deliberately no fallback: if the HIP library is missing or does not
export the expected ABI the import of any operator fails loudly.
"""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# DIFFORMER_HIP_LIB: another build of the SAME ABI (A/B kernel experiments); the default is the in-tree build
LIB_PATH = os.environ.get("DIFFORMER_HIP_LIB") or os.path.join(_HERE, "lib", "libdifformer_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_hip.h"))
# the attention-map library (C ABI: include/difformer_maps.h), loaded on first use by load_maps()
MAPS_LIB_PATH = os.path.join(_HERE, "lib", "libdifformer_maps.so")
MAPS_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_maps.h"))
# the edge-attention library (C ABI: include/difformer_edges.h), loaded on first use by load_edges()
EDGES_LIB_PATH = os.path.join(_HERE, "lib", "libdifformer_edges.so")
EDGES_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_edges.h"))
# the k-nearest-neighbour graph library (C ABI: include/difformer_knn.h), loaded on first use by load_knn()
KNN_LIB_PATH = os.path.join(_HERE, "lib", "libdifformer_knn.so")
KNN_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_knn.h"))
# the slot-order library of the packed sliced schedule (C ABI: include/difformer_slots.h), loaded on first use by load_slots()
SLOTS_LIB_PATH = os.path.join(_HERE, "lib", "libdifformer_slots.so")
SLOTS_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_slots.h"))
# the evaluation-metric library (C ABI: include/difformer_metrics.h), loaded on first use by load_metrics()
METRICS_LIB_PATH = os.path.join(_HERE, "lib", "libdifformer_metrics.so")
METRICS_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_metrics.h"))
# the training-loss library (C ABI: include/difformer_loss.h), loaded on first use by load_loss()
LOSS_LIB_PATH = os.path.join(_HERE, "lib", "libdifformer_loss.so")
LOSS_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_loss.h"))
# the optimiser library (C ABI: include/difformer_adam.h), loaded on first use by load_adam()
ADAM_LIB_PATH = os.path.join(_HERE, "lib", "libdifformer_adam.so")
ADAM_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_adam.h"))
# the graph read-out library (C ABI: include/difformer_readout.h), loaded on first use by load_readout()
READOUT_LIB_PATH = os.path.join(_HERE, "lib", "libdifformer_readout.so")
READOUT_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_readout.h"))
# the batched neighbour-graph library (C ABI: include/difformer_nbr.h), loaded on first use by load_nbr()
NBR_LIB_PATH = os.path.join(_HERE, "lib", "libdifformer_nbr.so")
NBR_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_nbr.h"))
# the snapshot-batch library (C ABI: include/difformer_snapshots.h), loaded on first use by load_snapshots()
SNAPSHOTS_LIB_PATH = os.path.join(_HERE, "lib", "libdifformer_snapshots.so")
SNAPSHOTS_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "difformer_snapshots.h"))

# The closed set of types the C ABI uses.  Every pointer is a c_void_p (device addresses arrive as integers), except the
# configuration struct; anything else in the header is an error, never a guess.
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double, "size_t": ctypes.c_size_t, "dif_stream_t": ctypes.c_void_p}
_NAME = r"dif_[a-z0-9_]+"


def _strip(text):
    """The header without its /* */ comments (#define lines are still there)."""
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _read_header(path):
    try:
        with open(path) as f:
            return _strip(f.read())
    except OSError as e:
        raise ImportError(f"difformer_amd: the C ABI header {path} is missing; the binding is derived from it") from e


def _defines(code, pattern):
    """`#define NAME n` / `#define NAME (n)` for the names that match `pattern` -> {NAME: n}."""
    found = re.findall(rf"^[ \t]*#[ \t]*define[ \t]+({pattern})[ \t]+\(?(-?\d+)\)?[ \t]*$", code, flags=re.M)
    if not found:
        raise ImportError(f"difformer_amd: {HEADER_PATH} defines no integer {pattern}")
    return {k: int(v) for k, v in found}


def _scalar(decl, where):
    """`[const] type [name]` -> ctypes type; anything that is not a scalar of the table raises."""
    words = [w for w in decl.split() if w != "const"]
    if not 1 <= len(words) <= 2 or words[0] not in _SCALARS or not re.fullmatch(r"\w+", words[-1]):
        raise ImportError(f"difformer_amd: {where}: cannot bind `{' '.join(decl.split())}`")
    return _SCALARS[words[0]]


def _struct_fields(code, name):
    """`typedef struct { type a, b; ... } name;` -> ctypes _fields_."""
    m = re.search(rf"typedef\s+struct\s*\{{([^{{}}]*)\}}\s*{name}\s*;", code)
    if m is None:
        raise ImportError(f"difformer_amd: {HEADER_PATH} does not declare struct {name}")
    fields = []
    for decl in filter(str.strip, m.group(1).split(";")):
        ctype, *fields_of_type = decl.split(None, 1)
        names = [f.strip() for f in "".join(fields_of_type).split(",")]
        if ctype not in _SCALARS or not all(re.fullmatch(r"[A-Za-z_]\w*", f) for f in names):
            raise ImportError(f"difformer_amd: {name} in {HEADER_PATH}: cannot bind `{' '.join(decl.split())}`")
        fields += [(f, _SCALARS[ctype]) for f in names]
    return fields


def _prototypes(code):
    """Every `ret dif_name(params);` of the comment-free header text -> {name: (restype, argtypes)}.  A `dif_name(` that
    is not such a prototype raises: a skipped function would be called with unchecked arguments."""
    code = re.sub(r"^[ \t]*#.*$", "", code, flags=re.M)
    code = re.sub(r"typedef\s+struct\s*\{[^{}]*\}\s*\w+\s*;|extern\s+\"C\"\s*\{", "", code)
    sigs = {}
    for stmt in code.split(";")[:-1]:                                # what follows the last ';' is left to the count below
        if not re.search(rf"{_NAME}\s*\(", stmt):
            continue
        m = re.fullmatch(rf"\s*([\w\s*]+?)\s*\b({_NAME})\s*\((.*)\)\s*", stmt, flags=re.S)
        if m is None:
            raise ImportError(f"difformer_amd: {HEADER_PATH}: not a prototype: `{' '.join(stmt.split())}`")
        ret, name, params = m.groups()
        where = f"{name} in {HEADER_PATH}"
        restype = ctypes.c_char_p if "".join(ret.split()) == "constchar*" else _scalar(ret, where)
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            if "*" not in p or re.search(r"[()\[\]]", p):           # by value; arrays and function pointers raise there
                argtypes.append(_scalar(p, where))
            elif re.match(r"\s*const\s+dif_tiny_cfg\s*\*", p):
                argtypes.append(ctypes.POINTER(TinyCfg))
            else:
                argtypes.append(ctypes.c_void_p)
        sigs[name] = (restype, argtypes)
    names = re.findall(rf"\b({_NAME})\s*\(", code)
    if len(names) != len(sigs):
        odd = sorted(n for n in set(names) if n not in sigs or names.count(n) > 1)
        raise ImportError(f"difformer_amd: {HEADER_PATH} has {len(names)} `dif_*(` for {len(sigs)} prototypes: {', '.join(odd)}")
    return sigs


_code = _read_header(HEADER_PATH)
ABI_VERSION = _defines(_code, "DIF_ABI_VERSION")["DIF_ABI_VERSION"]
ERROR_CODES = _defines(_code, r"DIF_E_\w+")                # name -> negative return code of a rejected argument


class TinyCfg(ctypes.Structure):
    """dif_tiny_cfg of include/difformer_hip.h."""
    _fields_ = _struct_fields(_code, "dif_tiny_cfg")


# name -> (restype, argtypes): include/difformer_hip.h is the only declaration of the entry points
SIGNATURES = _prototypes(_code)

# ... and include/difformer_maps.h of the second library's
_maps_code = _read_header(MAPS_HEADER_PATH)
MAPS_VERSION = _defines(_maps_code, "DIF_MAPS_VERSION")["DIF_MAPS_VERSION"]
MAPS_SIGNATURES = _prototypes(_maps_code)

# ... and include/difformer_edges.h of the third's
_edges_code = _read_header(EDGES_HEADER_PATH)
EDGES_VERSION = _defines(_edges_code, "DIF_EDGES_VERSION")["DIF_EDGES_VERSION"]
EDGES_SIGNATURES = _prototypes(_edges_code)

# ... and include/difformer_knn.h of the fourth's
_knn_code = _read_header(KNN_HEADER_PATH)
KNN_VERSION = _defines(_knn_code, "DIF_KNN_VERSION")["DIF_KNN_VERSION"]
KNN_SIGNATURES = _prototypes(_knn_code)

# ... and include/difformer_slots.h of the fifth's
_slots_code = _read_header(SLOTS_HEADER_PATH)
SLOTS_VERSION = _defines(_slots_code, "DIF_SLOTS_VERSION")["DIF_SLOTS_VERSION"]
SLOTS_SIGNATURES = _prototypes(_slots_code)

# ... and include/difformer_metrics.h of the sixth's
_metrics_code = _read_header(METRICS_HEADER_PATH)
METRICS_VERSION = _defines(_metrics_code, "DIF_METRICS_VERSION")["DIF_METRICS_VERSION"]
METRICS_SIGNATURES = _prototypes(_metrics_code)

# ... and include/difformer_loss.h of the seventh's
_loss_code = _read_header(LOSS_HEADER_PATH)
LOSS_VERSION = _defines(_loss_code, "DIF_LOSS_VERSION")["DIF_LOSS_VERSION"]
LOSS_CONSTANTS = _defines(_loss_code, r"DIF_LOSS_(?:ROWS|TARGET|RECORD)_\w+")      # rows_kind / target_type codes, record size
LOSS_SIGNATURES = _prototypes(_loss_code)

# ... and include/difformer_adam.h of the eighth's
_adam_code = _read_header(ADAM_HEADER_PATH)
ADAM_VERSION = _defines(_adam_code, "DIF_ADAM_VERSION")["DIF_ADAM_VERSION"]
ADAM_CONSTANTS = _defines(_adam_code, r"DIF_ADAM_(?:MAX_TENSORS|CHUNK|TABLE_FIELDS|TICKET_BYTES)")   # launch geometry, table row, tickets
ADAM_SIGNATURES = _prototypes(_adam_code)

# ... and include/difformer_readout.h of the ninth's
_readout_code = _read_header(READOUT_HEADER_PATH)
READOUT_VERSION = _defines(_readout_code, "DIF_READOUT_VERSION")["DIF_READOUT_VERSION"]
READOUT_CONSTANTS = _defines(_readout_code, r"DIF_READOUT_(?:ADD|MEAN|MAX|MAX_COLUMNS)")      # mode codes, the column limit
READOUT_SIGNATURES = _prototypes(_readout_code)

# ... and include/difformer_nbr.h of the tenth's
_nbr_code = _read_header(NBR_HEADER_PATH)
NBR_VERSION = _defines(_nbr_code, "DIF_NBR_VERSION")["DIF_NBR_VERSION"]
NBR_CONSTANTS = _defines(_nbr_code, r"DIF_NBR_MAX_(?:COLUMNS|K|CAP)")      # the limits of the batched kernels
NBR_SIGNATURES = _prototypes(_nbr_code)

# ... and include/difformer_snapshots.h of the eleventh's
_snapshots_code = _read_header(SNAPSHOTS_HEADER_PATH)
SNAPSHOTS_VERSION = _defines(_snapshots_code, "DIF_SNAP_VERSION")["DIF_SNAP_VERSION"]
SNAPSHOTS_CONSTANTS = _defines(_snapshots_code, r"DIF_SNAP_RECORD_FIELDS")      # int64 words of a snapshot record
SNAPSHOTS_SIGNATURES = _prototypes(_snapshots_code)

_lib = None
_maps = None
_edges = None
_knn = None
_slots = None
_metrics = None
_loss = None
_adam = None
_readout = None
_nbr = None
_snapshots = None


class DifformerHipError(RuntimeError):
    """A C-ABI call returned non-zero (argument rejected or HIP runtime failure)."""

    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


def _single_hip_runtime():
    """Two HIP runtimes in one process (torch's bundled one + a system one) do not share
    streams or allocations; refuse to run in that state."""
    try:
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    except OSError:
        return
    if len(paths) > 1:
        raise ImportError(f"difformer_amd: more than one HIP runtime mapped: {sorted(paths)}; "
                          "import torch before difformer_amd so that both share torch's libamdhip64")


def load():
    """Load the shared library once; raise ImportError with build instructions if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"difformer_amd: HIP extension not built ({LIB_PATH} missing). Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C difformer_amd/csrc`. "
            "There is no CPU / eager fallback.")
    import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first so the SONAME is shared)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"difformer_amd: {LIB_PATH} does not export {name}; rebuild it") from e
        fn.restype, fn.argtypes = res, args
    ver = lib.dif_version()
    if ver != ABI_VERSION:
        raise ImportError(f"difformer_amd: ABI version mismatch (library {ver}, host {ABI_VERSION}); rebuild")
    _single_hip_runtime()
    _lib = lib
    return lib


def _load_side(path, signatures, version_fn, version):
    """One of the small libraries next to libdifformer_hip.so (after it: one HIP runtime, checked there); same rules as load()."""
    load()
    if not os.path.exists(path):
        raise ImportError(
            f"difformer_amd: HIP extension not built ({path} missing). Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C difformer_amd/csrc`. "
            "There is no CPU / eager fallback.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"difformer_amd: {path} does not export {name}; rebuild it") from e
        fn.restype, fn.argtypes = res, args
    ver = getattr(lib, version_fn)()
    if ver != version:
        raise ImportError(f"difformer_amd: version mismatch of {path} (library {ver}, host {version}); rebuild")
    return lib


def load_maps():
    """Load libdifformer_maps.so once."""
    global _maps
    if _maps is None:
        _maps = _load_side(MAPS_LIB_PATH, MAPS_SIGNATURES, "dif_maps_version", MAPS_VERSION)
    return _maps


def load_edges():
    """Load libdifformer_edges.so once."""
    global _edges
    if _edges is None:
        _edges = _load_side(EDGES_LIB_PATH, EDGES_SIGNATURES, "dif_edges_version", EDGES_VERSION)
    return _edges


def load_knn():
    """Load libdifformer_knn.so once."""
    global _knn
    if _knn is None:
        _knn = _load_side(KNN_LIB_PATH, KNN_SIGNATURES, "dif_knn_version", KNN_VERSION)
    return _knn


def load_slots():
    """Load libdifformer_slots.so once."""
    global _slots
    if _slots is None:
        _slots = _load_side(SLOTS_LIB_PATH, SLOTS_SIGNATURES, "dif_slots_version", SLOTS_VERSION)
    return _slots


def load_metrics():
    """Load libdifformer_metrics.so once."""
    global _metrics
    if _metrics is None:
        _metrics = _load_side(METRICS_LIB_PATH, METRICS_SIGNATURES, "dif_metrics_version", METRICS_VERSION)
    return _metrics


def load_loss():
    """Load libdifformer_loss.so once."""
    global _loss
    if _loss is None:
        _loss = _load_side(LOSS_LIB_PATH, LOSS_SIGNATURES, "dif_loss_version", LOSS_VERSION)
    return _loss


def load_adam():
    """Load libdifformer_adam.so once."""
    global _adam
    if _adam is None:
        _adam = _load_side(ADAM_LIB_PATH, ADAM_SIGNATURES, "dif_adam_version", ADAM_VERSION)
    return _adam


def load_readout():
    """Load libdifformer_readout.so once."""
    global _readout
    if _readout is None:
        _readout = _load_side(READOUT_LIB_PATH, READOUT_SIGNATURES, "dif_readout_version", READOUT_VERSION)
    return _readout


def load_nbr():
    """Load libdifformer_nbr.so once."""
    global _nbr
    if _nbr is None:
        _nbr = _load_side(NBR_LIB_PATH, NBR_SIGNATURES, "dif_nbr_version", NBR_VERSION)
    return _nbr


def load_snapshots():
    """Load libdifformer_snapshots.so once."""
    global _snapshots
    if _snapshots is None:
        _snapshots = _load_side(SNAPSHOTS_LIB_PATH, SNAPSHOTS_SIGNATURES, "dif_snap_version", SNAPSHOTS_VERSION)
    return _snapshots


def check_maps(rc, what):
    """check() for a call into libdifformer_maps.so: the message comes from that library."""
    if rc != 0:
        msg = load_maps().dif_maps_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def check_edges(rc, what):
    """check() for a call into libdifformer_edges.so: the message comes from that library."""
    if rc != 0:
        msg = load_edges().dif_edges_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def check_knn(rc, what):
    """check() for a call into libdifformer_knn.so: the message comes from that library."""
    if rc != 0:
        msg = load_knn().dif_knn_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def check_slots(rc, what):
    """check() for a call into libdifformer_slots.so: the message comes from that library."""
    if rc != 0:
        msg = load_slots().dif_slots_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def check_metrics(rc, what):
    """check() for a call into libdifformer_metrics.so: the message comes from that library."""
    if rc != 0:
        msg = load_metrics().dif_metrics_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def check_loss(rc, what):
    """check() for a call into libdifformer_loss.so: the message comes from that library."""
    if rc != 0:
        msg = load_loss().dif_loss_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def check_adam(rc, what):
    """check() for a call into libdifformer_adam.so: the message comes from that library."""
    if rc != 0:
        msg = load_adam().dif_adam_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def check_readout(rc, what):
    """check() for a call into libdifformer_readout.so: the message comes from that library."""
    if rc != 0:
        msg = load_readout().dif_readout_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def check_nbr(rc, what):
    """check() for a call into libdifformer_nbr.so: the message comes from that library."""
    if rc != 0:
        msg = load_nbr().dif_nbr_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def check_snapshots(rc, what):
    """check() for a call into libdifformer_snapshots.so: the message comes from that library."""
    if rc != 0:
        msg = load_snapshots().dif_snap_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def check(rc, what):
    if rc != 0:
        msg = load().dif_last_error()
        raise DifformerHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)
