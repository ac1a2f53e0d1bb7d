"""The host kit of CopterVecEnv's rollout wrappers: what every wrapper does between its arguments and one call of
libcopterstep.so -- io blocks, argument coercion, scalar checks, the values checked on the host and uploaded once, the
output buffers and the launch.  Plain functions on an env (anything with device, num_envs, _lib, _ctx and _stream());
this module imports _lib, numpy and, lazily, torch, and every family module imports this one ("the host
side").  step(), reset() and the served path do not go through it."""
import ctypes as C
import math

import numpy as np

from . import _lib


def _torch():
    import torch
    return torch


# -- io blocks ---------------------------------------------------------------------------------------------------------
_MEMBERS = {}      # struct class -> (its members' names, its size)


def block(struct_cls, **fields):
    """An io block of the C ABI: struct_size set, the given members assigned (pointers as data_ptr() values or None)."""
    known = _MEMBERS.get(struct_cls)
    if known is None:
        known = _MEMBERS[struct_cls] = (frozenset(name for name, _ in struct_cls._fields_), C.sizeof(struct_cls))
    if not fields.keys() <= known[0]:
        raise AttributeError("%s has no member %r" % (struct_cls.__name__, sorted(fields.keys() - known[0])[0]))
    b = struct_cls(**fields)
    b.struct_size = known[1]
    return b


def out_dtype(dtype):
    """The dtype of a derivative's outputs: torch.float64 (None) or torch.float32."""
    torch = _torch()
    dtype = torch.float64 if dtype is None else dtype
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("dtype must be torch.float64 or torch.float32")
    return dtype


def dtype_code(dtype):
    """The CS_JAC_F64 / CS_JAC_F32 code of an out_dtype() (None: float64)."""
    return _lib.JAC_F32 if dtype == _torch().float32 else _lib.JAC_F64


# -- arguments ---------------------------------------------------------------------------------------------------------
def tensor(env, v, shape, dtype, name, keep, *, host=True, floating=False, strict=False, foreign=True,
           non_blocking=False, note=""):
    """The argument `v` as a contiguous tensor of `shape` and `dtype` on env.device, appended to `keep` (alive until the
    stream has consumed it) and returned.  `name` is what the messages call it.  The rule is the call site's:
    host=False: torch tensors only (with `floating`, type and dtype are checked before the shape, in one message);
    floating: the dtype must be floating-point;  strict (the filters' rule): the messages say what they got, and a host
    array is checked as NumPy sees it (dtype kind "f") and converted on the host;  foreign=False: a tensor on another
    device is refused, not moved;  non_blocking: passed to the move;  note: appended to the shape in the shape message."""
    torch = _torch()
    dev = env.device
    is_tensor = isinstance(v, torch.Tensor)
    if not host and (not is_tensor or (floating and not v.dtype.is_floating_point)):
        raise ValueError("%s must be a floating-point torch tensor of shape %s" % (name, shape))
    a = None
    if is_tensor:
        t = v
    elif strict:
        t, a = None, np.asarray(v)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
    got = a.shape if t is None else tuple(t.shape)
    if got != shape:
        raise ValueError("%s must have shape %s%s, got %s" % (name, shape, note, got))
    if floating:
        if t is None:
            if a.dtype.kind != "f":
                raise ValueError("%s must be a floating-point array, got dtype %s" % (name, a.dtype))
        elif not t.dtype.is_floating_point:
            raise ValueError("%s must be a floating-point tensor, got %s" % (name, t.dtype) if strict else
                             "%s must be a floating-point array" % name)
    if is_tensor and not foreign and t.device != dev:
        raise ValueError("%s must be on %s, got %s" % (name, dev, t.device))
    if t is None:
        np_dtype = np.float64 if dtype == torch.float64 else np.float32
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(dev)
    else:
        t = t.detach().to(device=dev, dtype=dtype, non_blocking=non_blocking).contiguous()
    keep.append(t)
    return t


def exact_vector(env, v, size, name, keep, wording, foreign=True):
    """A parameter vector that must already be a [size] float32 torch tensor (with foreign=False: on env.device; else it
    is moved there): one check, no conversion, the call site's message -- `wording` with %(name)s, %(size)d, %(device)s
    and %(got)s.  Contiguous, appended to `keep` and returned."""
    torch = _torch()
    dev = env.device
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != (size,) \
            or not (foreign or v.device == dev):
        raise ValueError(wording % {"name": name, "size": size, "device": dev,
                                    "got": getattr(v, "shape", type(v).__name__)})
    t = v.detach().to(dev).contiguous()
    keep.append(t)
    return t


def check_tape(env, source, *tapes):
    """A backward's tape, (tensor, name, shape, dtype) each: contiguous device tensors as `source` returned them."""
    torch = _torch()
    for t, name, shape, dt in tapes:
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a device tensor of shape %s (%s' result)" % (name, shape, source))
        if tuple(t.shape) != shape:
            raise ValueError("%s must have shape %s, got %s" % (name, shape, tuple(t.shape)))
        if t.dtype != dt or t.device != env.device or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor on %s" % (name, dt, env.device))


def int_in(v, name, lo, hi, what, ok=None):
    """v as an int: an int (no bool) with lo <= v < hi (None: no bound) that passes ok(v), else "<name> must be <what>,
    got <v>"."""
    if (not isinstance(v, (int, np.integer)) or isinstance(v, bool) or (lo is not None and int(v) < lo)
            or (hi is not None and int(v) >= hi) or (ok is not None and not ok(int(v)))):
        raise ValueError("%s must be %s, got %r" % (name, what, v))
    return int(v)


U32 = 1 << 32
IN_U32 = "an int in [0, 2**32)"      # int_in(v, name, 0, U32, IN_U32): a nonce, a stream, a pair base


def finite(v, name, lo=None, above=False):
    """v as a finite float: >= lo (above=True: > lo; lo=None: any), else "<name> must be finite[ and >= <lo>], got <v>"."""
    f = float(v)
    if lo is None:
        if not math.isfinite(f):
            raise ValueError("%s must be finite, got %r" % (name, v))
    elif not (f > lo if above else f >= lo) or f == float("inf"):
        raise ValueError("%s must be finite and %s %s, got %r" % (name, ">" if above else ">=", lo, v))
    return f


# -- values checked on the host and uploaded once ------------------------------------------------------------------------
def uploaded(env, slot, check, given=None):
    """The device copies of the small arrays an entry point shares among every env and step (weights, a filter's model,
    a knot table): check() returns the host arrays to upload (None entries stay None), checked; the copies are kept in
    env._uploaded[slot] and reused while the arrays' bytes are equal (a driver passes them with every iteration or
    chunk).  given: the caller's objects -- when they are all device tensors they are recognised by identity, version
    and address (the same, unmodified tensors as in the slot's last call cost no device-to-host copy and no check) and
    checked on the host once when they are new."""
    caches = env.__dict__.get("_uploaded")
    if caches is None:
        caches = env._uploaded = {}
    cache = caches.get(slot)
    ident = None
    if given is not None:
        Tensor = _torch().Tensor
        if all(isinstance(m, Tensor) for m in given):
            ident = tuple((id(m), m._version, m.data_ptr()) for m in given)
            if cache is not None and cache[2] == ident:
                return cache[1]
    model = check()
    key = [None if a is None else a.tobytes() for a in model]
    if cache is None or cache[0] != key:
        torch = _torch()
        cache = (key, [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(env.device) for a in model])
    elif ident is None and cache[2] is None:
        return cache[1]
    # (the caller's tensors are kept alive with their identity, so that an id cannot be reused by another tensor)
    caches[slot] = (cache[0], cache[1], ident, given if ident is not None else None)
    return cache[1]


# -- outputs and the launch ----------------------------------------------------------------------------------------------
def empty(env, shape, dtype):
    """An output buffer on env.device.  (torch.empty is looked up at call time and given nothing but a dtype and a
    device: tests/guarded_outputs.py replaces it for a block.)"""
    return _torch().empty(shape, dtype=dtype, device=env.device)


def rollout_cache(env, key, make):
    """The env's cached output buffers of one entry point and shape: make() allocates them on first use."""
    cache = getattr(env, "_rollout_out", None)
    if cache is None:
        cache = env._rollout_out = {}
    out = cache.get(key)
    if out is None:
        out = cache[key] = make()
    return out


def launch(env, entry, *blocks, keep):
    """One library call on the env's device and current stream: entry(ctx, the blocks by reference (None: a NULL block),
    stream), its status checked; `keep` -- what the call reads -- stays alive in env._keep.  (The entry point is looked
    up by name at call time: tests/null_outputs.py replaces the attribute.)"""
    refs = [None if b is None else C.byref(b) for b in blocks]
    with _torch().cuda.device(env.device):
        rc = getattr(env._lib, entry)(env._ctx, *refs, env._stream())
        if rc != 0:
            _lib.check(rc)
    env._keep = keep
