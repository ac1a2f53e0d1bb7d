"""tests/guarded_outputs.py catches what it claims to, with device="cpu" standing in for the GPU: a fake "wrapper"
allocates its outputs with torch.empty(..., device="cpu") as gym_copter_amd/vecenv.py does on its device, and a fake
"kernel" fills them -- exactly, past an end, before the start, with a hole, or into a tensor of its own.  Plus the list
of entry points tests/test_gpu_output_bounds.py covers against the methods CopterVecEnv has."""
import ast
import os

import pytest

torch = pytest.importorskip("torch")

from guarded_outputs import ALIGN, FILL, band_bytes, guarded      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K = 65, 3
DTYPES = [torch.float64, torch.float32, torch.int32, torch.uint8, torch.bool]
SHAPES = [(N,), (K, N, 12, 12), (K, N, 1)]


def _fill_exactly(t):
    """What a correct kernel leaves: every element written, with a value that is not the fill."""
    if t.dtype == torch.bool:
        t.view(torch.uint8).copy_((torch.arange(t.numel()) % 2).to(torch.uint8).view(t.shape))
    elif t.dtype.is_floating_point:
        t.copy_(torch.arange(t.numel(), dtype=torch.float64).view(t.shape) - 7.5)
    else:
        t.copy_((torch.arange(t.numel()) % 100).view(t.shape))
    return t


def _wrapper(shape, dtype):
    """A stand-in for a CopterVecEnv method: allocates as the wrappers do, looked up at call time."""
    import torch as T
    return T.empty(shape, dtype=dtype, device="cpu")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_exact_fill_passes_and_the_layout_follows_the_rule(dtype, shape):
    real = torch.empty
    x = torch.linspace(-1, 1, 37, dtype=torch.float64)
    x[5] = float("nan")
    with guarded(N, device="cpu") as g:
        g.freeze(x=x)
        out = _fill_exactly(_wrapper(shape, dtype))
        host = torch.empty(shape, dtype=dtype)                     # no device=: passes through untouched
        pinned = torch.empty(4, dtype=dtype, device="cpu", pin_memory=False)    # not a wrapper's call: passes through
    assert torch.empty is real
    assert len(g.allocations) == 1
    a = g.allocations[0]
    nbytes = out.numel() * out.element_size()
    assert out.dtype == dtype and tuple(out.shape) == shape and out.is_contiguous()
    assert (a.dtype, a.shape, a.nbytes, a.order) == (dtype, shape, nbytes, 0)
    want = max(4096, -(-256 * nbytes // N))
    want = -(-want // 512) * 512
    assert a.front == a.back == want == band_bytes(nbytes, N)
    assert a.front % ALIGN == 0 and out.data_ptr() % 512 == 0
    assert a.backing.dtype == torch.uint8 and a.backing.numel() == a.front + nbytes + a.back
    assert out.data_ptr() == a.backing.data_ptr() + a.front == a.ptr
    assert host.data_ptr() != out.data_ptr() and g._allocation_of(host) is None and g._allocation_of(pinned) is None
    g.assert_bands_intact()
    g.assert_fully_written(out)
    g.assert_fully_written({"a": [out, None], "b": (out[..., 0],)})
    g.assert_inputs_unchanged()


def test_band_rule_values():
    """256 envs' worth, a floor of 4096 bytes, rounded up to 512."""
    assert band_bytes(0, 1) == 4096 and band_bytes(64, 64) == 4096
    assert band_bytes(8 * 12 * 65, 65) == 24576                   # [65,12] float64: 256 x 96 bytes
    assert band_bytes(4 * 10 * 191, 191) == 10240                 # [191,10] float32: 256 x 40 bytes
    assert band_bytes(4 * 191, 191) == 4096
    assert band_bytes(3 * 191 * 1152, 191) == 884736 and band_bytes(8 * 7, 3) == 5120       # 4778.7 -> 5120
    assert band_bytes(3 * 191 * 1152, 191) < 1 << 20              # [3,N,12,12] float64: still under a megabyte


def _call(dtype, shape, spoil):
    """One guarded fake call: the payload filled exactly, then `spoil(out, allocation)`."""
    with guarded(N, device="cpu") as g:
        out = _fill_exactly(_wrapper(shape, dtype))
        first = _fill_exactly(_wrapper((N,), torch.float32))       # (a second allocation: the message names the right one)
        spoil(out, g.allocations[0])
    return g, (first, out)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("where", ["one_past_the_end", "far_edge_of_the_back_band", "one_before_the_start",
                                   "far_edge_of_the_front_band"])
def test_a_write_outside_the_payload_fails_on_the_correct_side(dtype, where):
    size = torch.empty((), dtype=dtype).element_size()

    def spoil(out, a):
        end = a.front + a.nbytes
        lo = {"one_past_the_end": end, "far_edge_of_the_back_band": end + a.back - size,
              "one_before_the_start": a.front - size, "far_edge_of_the_front_band": 0}[where]
        a.backing[lo:lo + size] = 1                                # one element, through the backing buffer
    g, result = _call(dtype, (K, N, 1), spoil)
    side = "back" if where in ("one_past_the_end", "far_edge_of_the_back_band") else "front"
    with pytest.raises(AssertionError, match=r"the %s band of allocation #0 \(shape \(3, 65, 1\)" % side) as e:
        g.assert_bands_intact()
    a = g.allocations[0]
    want = {"one_past_the_end": "bytes 0 .. %d past the payload's end" % (size - 1),
            "far_edge_of_the_back_band": "bytes %d .. %d past the payload's end" % (a.back - size, a.back - 1),
            "one_before_the_start": "bytes %d .. 1 before the payload's start" % size,
            "far_edge_of_the_front_band": "bytes %d .. %d before the payload's start" % (a.front, a.front - size + 1)}
    assert want[where] in str(e.value), str(e.value)
    g.assert_fully_written(result)                                  # (the payloads themselves are whole)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_an_unwritten_element_fails_fully_written(dtype):
    def spoil(out, a):
        size = out.element_size()
        at = a.front + ((1 * N + 7) * 12 + 5) * size
        a.backing[at:at + size] = FILL
    g, result = _call(dtype, (K, N, 12), spoil)
    g.assert_bands_intact()
    with pytest.raises(AssertionError, match=r"1 of 2340 elements were not written, the first at index \[1, 7, 5\]"):
        g.assert_fully_written(result)
    # through a strided view of the tensor as well (the flag columns of an interleaved array are such views)
    with pytest.raises(AssertionError, match=r"1 of 195 elements were not written, the first at index \[1, 7\]"):
        g.assert_fully_written([result[1][:, :, 5]])
    g.assert_fully_written([result[1][:, :, 4]])
    g.assert_fully_written(result, except_=(result[1],))           # a documented exemption is skipped


def test_a_partly_filled_element_counts_as_written():
    """Only an element whose bytes ALL hold the fill is unwritten: a float64 with one such byte is a value."""
    def spoil(out, a):
        a.backing[a.front + 3] = FILL
    g, result = _call(torch.float64, (N,), spoil)
    g.assert_fully_written(result)


def test_a_tensor_the_helper_did_not_allocate_fails_fully_written():
    with guarded(N, device="cpu") as g:
        out = _fill_exactly(_wrapper((N,), torch.float32))
    own = torch.zeros(N)
    with pytest.raises(AssertionError, match="does not lie inside a guarded allocation"):
        g.assert_fully_written((out, own))
    # a view that starts inside a payload and runs past its end is no output of the helper's either
    a = g.allocations[0]
    long = a.backing[a.front:a.front + a.nbytes + 4].view(torch.float32)
    with pytest.raises(AssertionError, match="does not lie inside a guarded allocation"):
        g.assert_fully_written(long)


def test_no_interception_fails_instead_of_passing_empty():
    with guarded(N, device="cpu") as g:
        out = torch.zeros(N)                                        # (a wrapper that stopped calling torch.empty)
    with pytest.raises(AssertionError, match="no allocation was intercepted"):
        g.assert_bands_intact()
    with pytest.raises(AssertionError, match="no allocation was intercepted"):
        g.assert_fully_written(out)
    with pytest.raises(AssertionError, match="no input was frozen"):
        g.assert_inputs_unchanged()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_one_changed_bit_of_an_input_fails_inputs_unchanged(dtype):
    x = _fill_exactly(torch.empty((K, N), dtype=dtype))
    y = torch.full((4,), float("nan"))
    with guarded(N, device="cpu") as g:
        g.freeze(x=x, y=y)
        _fill_exactly(_wrapper((N,), torch.float32))
        g.assert_inputs_unchanged()                                 # (NaNs compare equal bit for bit)
        x.view(torch.uint8).view(-1)[x.element_size() * 70] ^= 1 if dtype != torch.bool else 2
    with pytest.raises(AssertionError, match=r"input 'x' \(shape \(3, 65\).* 1 elements differ, the first at flat index 70"):
        g.assert_inputs_unchanged()


def test_another_fill_byte():
    with guarded(N, device="cpu", fill=0x5A) as g:
        out = _wrapper((N,), torch.uint8)
        out.fill_(FILL)                                             # 0xA5 is a value under this guard
    assert int(g.allocations[0].backing[0]) == 0x5A
    g.assert_bands_intact()
    g.assert_fully_written(out)


# ---------------------------------------------------------------------------------------------------------------------
# every entry point is in tests/test_gpu_output_bounds.py
# ---------------------------------------------------------------------------------------------------------------------
def _entry_points():
    """The public methods of CopterVecEnv that the contract covers: the class's own attributes (no device, no library),
    whether a method is defined in the class body or bound there from its family's module."""
    import gym_copter_amd
    names = [n for n, v in vars(gym_copter_amd.CopterVecEnv).items() if callable(v)]
    return {n for n in names if n.startswith(("rollout_", "es_")) or n in ("gae", "ppo_grad", "mlp_param_grad",
                                                                          "step_jacobian", "step_many")}


def _module_functions(module):
    """(name -> ast.FunctionDef of the test module's top-level functions, alias -> module for its `import x as alias`)"""
    tree = ast.parse(open(os.path.join(ROOT, "tests", module + ".py")).read())
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    aliases = {a.asname or a.name: a.name for n in tree.body if isinstance(n, ast.Import) for a in n.names}
    return funcs, aliases


def _methods_called(module, test):
    """The attribute names called in `test` of tests/<module>.py, in the module's own helpers it calls (one level) and
    in the helpers of another test module it calls as <alias>.<helper>(...)."""
    funcs, aliases = _module_functions(module)
    assert test in funcs and test.startswith("test_"), (module, test)
    calls = [n for n in ast.walk(funcs[test]) if isinstance(n, ast.Call)]
    for h in {n.func.id for n in calls if isinstance(n.func, ast.Name)} & set(funcs):
        calls += [n for n in ast.walk(funcs[h]) if isinstance(n, ast.Call)]
    called = {n.func.attr for n in calls if isinstance(n.func, ast.Attribute)}
    for n in calls:
        f = n.func
        if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and aliases.get(f.value.id, "").startswith("test_"):
            other = _module_functions(aliases[f.value.id])[0]
            if f.attr in other:
                called |= {c.func.attr for c in ast.walk(other[f.attr]) if isinstance(c, ast.Call)
                           and isinstance(c.func, ast.Attribute)}
    return called


def test_every_entry_point_is_covered():
    import test_gpu_output_bounds as B
    have = _entry_points()
    assert len(have) >= 27 and {"step_many", "rollout_rts", "es_gradient", "gae", "rollout_pf", "rollout_lqg",
                                "rollout_ukf"} <= have, sorted(have)
    assert set(B.SKIPPED) <= have and all(reason for reason in B.SKIPPED.values())
    assert not set(B.COVERED) & set(B.SKIPPED)
    missing = have - set(B.COVERED) - set(B.SKIPPED)
    assert not missing, "entry points without a guarded-output test named in tests/test_gpu_output_bounds.py: %s" \
        % sorted(missing)
    stale = set(B.COVERED) - have
    assert not stale, "tests/test_gpu_output_bounds.py lists methods CopterVecEnv does not have: %s" % sorted(stale)
    # the list is not a declaration only: every covered method is called on an env in the test named for it -- a test of
    # tests/test_gpu_output_bounds.py, or "<module>::<test>" for a family whose guarded test lives with its own tests
    for method, test in B.COVERED.items():
        module, name = test.split("::") if "::" in test else ("test_gpu_output_bounds", test)
        assert method in _methods_called(module, name), "%s::%s does not call env.%s" % (module, name, method)
        funcs = _module_functions(module)[0]
        entered = [i.context_expr for w in ast.walk(funcs[name]) if isinstance(w, ast.With) for i in w.items]
        assert module == "test_gpu_output_bounds" or any(
            isinstance(e, ast.Call) and isinstance(e.func, ast.Name) and e.func.id == "guarded" for e in entered), \
            "%s::%s never enters `with guarded(...)`" % (module, name)
