"""Guarded output buffers for the memory contract of CopterVecEnv's entry points (tests/test_gpu_output_bounds.py): no
entry point writes outside the arrays it is given, it writes every element of every output, and it leaves its inputs
unchanged.

CopterVecEnv's wrappers allocate every output with torch.empty(..., device=<the env's>), looked up at call time
(gym_copter_amd/_wire.py's empty(); step_many and _rollout in vecenv.py).  `with guarded(N) as guard:` replaces
torch.empty for the block: an allocation on the guarded device becomes the middle of one uint8 backing tensor filled with
the byte 0xA5, with a band of the same fill in front of it and behind it.  A store past either end of an output lands in
a band and stays visible; an element nobody stored still holds the fill.

    with guarded(env.num_envs) as guard:
        guard.freeze(actions=actions)
        result = env.rollout_states(actions)
    torch.cuda.synchronize()
    guard.assert_bands_intact()
    guard.assert_fully_written(result)
    guard.assert_inputs_unchanged()

Band size: 256 envs' worth of the tensor (256 * nbytes / N bytes), at least 4096 bytes, rounded up to a multiple of 512.
256 lanes cover every lane past the end of the last workgroup at every block size the library launches (64 lanes per
wavefront, at most four wavefronts per workgroup).  The front band being a multiple of 512 bytes and the backing tensor
starting on a 512-byte boundary, the payload keeps the alignment torch's caching allocator gives (kernels load tapes as
double2).

0xA5 is a value no output takes: flags and ok are 0 or 1, a status is at most 2, the step Jacobian's branch bits at most
127, counts and indices are small, and the float patterns are -2.9e-16 (float32) and about -1e-129 (float64).  A test
whose output can legitimately hold that byte passes another `fill`."""
import collections
from unittest import mock

import numpy as np

FILL = 0xA5
ALIGN = 512
BAND_ENVS = 256
BAND_FLOOR = 4096

Allocation = collections.namedtuple("Allocation", "order backing front nbytes back dtype shape ptr")


def band_bytes(nbytes, num_envs):
    """Bytes of one guard band of a tensor of `nbytes` bytes among `num_envs` envs."""
    need = max(BAND_FLOOR, -(-BAND_ENVS * nbytes // num_envs))
    return -(-need // ALIGN) * ALIGN


def _int_view(t):
    """t's elements as integers of the same size, bit for bit (any strides): NaNs compare, and so do the bytes of a bool
    that are neither 0 nor 1."""
    import torch
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _walk(obj, path="result"):
    """(path, tensor) of every tensor in a wrapper's return value: tuples, named tuples, lists and dicts; None is skipped."""
    import torch
    if isinstance(obj, torch.Tensor):
        yield path, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _walk(v, "%s[%r]" % (path, k))
    elif isinstance(obj, (tuple, list)):
        names = getattr(obj, "_fields", None)
        for i, v in enumerate(obj):
            yield from _walk(v, "%s.%s" % (path, names[i]) if names else "%s[%d]" % (path, i))
    elif obj is not None:
        raise AssertionError("%s: cannot walk a %s" % (path, type(obj).__name__))


class Guard:
    def __init__(self, num_envs, device="cuda", fill=FILL):
        import torch
        if not isinstance(num_envs, int) or num_envs < 1:
            raise ValueError("num_envs must be an int >= 1, got %r" % (num_envs,))
        if not 0 <= fill <= 255:
            raise ValueError("fill must be a byte, got %r" % (fill,))
        self.num_envs, self.fill = num_envs, fill
        self.device_type = torch.device(device).type
        self.allocations = []
        self.frozen = {}
        self._patch = None

    # -- the replacement of torch.empty -------------------------------------------------------------------------------
    def _guards(self, kwargs):
        """True for a call this guard replaces: device= names the guarded device type, and nothing but a dtype comes with
        it (a layout, pin_memory, out=, memory_format or requires_grad is none of the wrappers' and passes through)."""
        import torch
        if kwargs.get("device") is None or set(kwargs) - {"device", "dtype"}:
            return False
        dev = kwargs["device"]
        dev = torch.device("cuda", dev) if isinstance(dev, int) else torch.device(dev)
        return dev.type == self.device_type

    def _empty(self, *size, **kwargs):
        import torch
        if not self._guards(kwargs):
            return self._real_empty(*size, **kwargs)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        shape = tuple(int(s) for s in size)
        dtype = kwargs.get("dtype") or torch.get_default_dtype()
        itemsize = self._real_empty((), dtype=dtype).element_size()
        count = 1
        for s in shape:
            count *= s
        nbytes = count * itemsize
        front = back = band_bytes(nbytes, self.num_envs)
        total = front + nbytes + back
        # (ALIGN - 1 spare bytes: the backing tensor proper starts on the next 512-byte boundary, wherever the allocator
        # put the block -- torch's caching allocator for device memory already does, the host allocator does not)
        raw = self._real_empty(total + ALIGN - 1, dtype=torch.uint8, device=kwargs["device"])
        raw.fill_(self.fill)
        skip = -raw.data_ptr() % ALIGN
        backing = raw[skip:skip + total]
        payload = backing[front:front + nbytes].view(dtype).view(shape)
        assert payload.is_contiguous() and payload.data_ptr() % ALIGN == 0 and payload.data_ptr() == backing.data_ptr() + front
        self.allocations.append(Allocation(len(self.allocations), backing, front, nbytes, back, dtype, shape,
                                           payload.data_ptr()))
        return payload

    def __enter__(self):
        import torch
        self._real_empty = torch.empty
        self._patch = mock.patch.object(torch, "empty", self._empty)
        self._patch.start()
        return self

    def __exit__(self, *exc):
        self._patch.stop()
        self._patch = None
        return False

    # -- the three checks ---------------------------------------------------------------------------------------------
    def assert_bands_intact(self):
        """Every byte of every front and back band still reads the fill."""
        assert self.allocations, "no allocation was intercepted: the guard checks nothing"
        for a in self.allocations:
            for side, lo, hi in (("front", 0, a.front), ("back", a.front + a.nbytes, a.front + a.nbytes + a.back)):
                band = a.backing[lo:hi]
                bad = (band != self.fill).nonzero()
                if bad.numel():
                    first, last = int(bad[0]), int(bad[-1])
                    if side == "front":
                        where = "bytes %d .. %d before the payload's start" % (a.front - first, a.front - last)
                    else:
                        where = "bytes %d .. %d past the payload's end" % (first, last)
                    raise AssertionError(
                        "the %s band of allocation #%d (shape %s, %s, %d bytes) was written: %d bytes touched, %s"
                        % (side, a.order, a.shape, a.dtype, a.nbytes, int(bad.numel()), where))

    def _allocation_of(self, t):
        ptr = t.data_ptr()
        extent = (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size() if t.numel() else 0
        for a in self.allocations:
            if a.ptr <= ptr and ptr + extent <= a.ptr + a.nbytes and (a.nbytes > 0 or ptr == a.ptr):
                return a
        return None

    def assert_fully_written(self, result, except_=()):
        """No element of any tensor in `result` still holds the fill in all its bytes; every such tensor lies inside a
        recorded payload.  except_: tensors of `result` (matched by identity) that the documentation says may be left
        as they were."""
        import torch
        assert self.allocations, "no allocation was intercepted: the guard checks nothing"
        found = list(_walk(result))
        assert found, "the result holds no tensor"
        for e in except_:
            assert any(e is t for _, t in found), "an except_ entry is not a tensor of the result"
        for path, t in found:
            a = self._allocation_of(t)
            assert a is not None, ("%s (shape %s, %s) does not lie inside a guarded allocation: it was not made by the "
                                   "intercepted torch.empty" % (path, tuple(t.shape), t.dtype))
            if any(e is t for e in except_) or t.numel() == 0:
                continue
            size = t.element_size()
            pattern = int.from_bytes(bytes([self.fill]) * size, "little", signed=True)
            if t.is_complex():
                raise AssertionError("%s: complex outputs are not supported" % path)
            unwritten = (_int_view(t) == pattern).reshape(-1).nonzero()
            if unwritten.numel():
                idx = [int(i) for i in np.unravel_index(int(unwritten[0, 0]), tuple(t.shape))] if t.dim() else []
                raise AssertionError("%s (allocation #%d, shape %s, %s): %d of %d elements were not written, the first at "
                                     "index %s" % (path, a.order, tuple(t.shape), t.dtype, int(unwritten.numel()),
                                                   t.numel(), idx))

    def refill(self, result):
        """Give the payloads under the tensors of `result` (an earlier call's return value) the fill again: the wrappers
        cache their output buffers, so a second call of one method on one env writes the first call's tensors."""
        for path, t in _walk(result):
            a = self._allocation_of(t)
            assert a is not None, "%s does not lie inside a guarded allocation" % path
            a.backing[a.front:a.front + a.nbytes].fill_(self.fill)

    def freeze(self, **tensors):
        """Keep a copy of the named input tensors for assert_inputs_unchanged()."""
        for name, t in tensors.items():
            assert name not in self.frozen, name
            self.frozen[name] = (t, t.detach().clone())

    def release(self):
        """Forget the frozen inputs (before the next call under the same guard)."""
        self.frozen = {}

    def assert_inputs_unchanged(self):
        import torch
        assert self.frozen, "no input was frozen"
        for name, (t, copy) in self.frozen.items():
            same = _int_view(t.detach()) == _int_view(copy)
            if not bool(same.all()):
                bad = (~same).reshape(-1).nonzero()
                raise AssertionError("input %r (shape %s, %s) was modified: %d elements differ, the first at flat index %d"
                                     % (name, tuple(t.shape), t.dtype, int(bad.numel()), int(bad[0, 0])))


def guarded(num_envs, device="cuda", fill=FILL):
    """The context manager: see the module's docstring."""
    return Guard(num_envs, device=device, fill=fill)
