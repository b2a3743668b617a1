"""tests/guarded.py without a GPU: the detector fires where it must and stays silent where it must not, the poison shows
through unwritten views, the seam covers every allocation call in the text of ops.py, and every workspace query that
text names has a driver in tests/test_gpu_guarded.py (the ratchet: no exemptions)."""
import math
import os
import re
import types

import pytest
import torch

from tests import guarded as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS_PATH = os.path.join(ROOT, "explicit-tf2-recommendation_amd", "ops.py")


def fake_ops():
    """a stand-in for the ops module: the two globals the seam swaps, and this file as the one whose frames are named"""
    return types.SimpleNamespace(torch=torch, lib=types.SimpleNamespace(
        rec_mmoe_workspace_bytes=lambda *a: 64, rec_mmoe_bwd_f32=lambda *a: 0), __file__=__file__)


def allocate_like_ops(ops, shape, dtype=torch.float32, call="empty"):
    return getattr(ops.torch, call)(shape, dtype=dtype, device="cpu")


def test_an_untouched_and_a_fully_written_allocation_pass():
    ops = fake_ops()
    with G.guarded(ops, 0xFF) as g:
        allocate_like_ops(ops, (3, 5))
        allocate_like_ops(ops, (7,)).fill_(1.0)
        ops.torch.empty_like(torch.ones(2, 3)).copy_(torch.ones(2, 3))
    assert len(g.allocations) == 3 and g.total_bytes() == 4 * (15 + 7 + 6)
    assert ops.torch is torch                              # the globals are back
    a = g.allocations[0]
    assert a.view.is_contiguous() and a.view.storage_offset() * a.view.element_size() == G.GUARD
    assert a.base.numel() == 2 * G.GUARD + 60 and a.frames[0].startswith("allocate_like_ops:")


@pytest.mark.parametrize("poison", [0xFF, 0x7F])
@pytest.mark.parametrize("side", ["before", "after"])
def test_a_write_one_element_outside_the_view_is_detected_and_named(poison, side):
    ops = fake_ops()
    with pytest.raises(G.GuardError) as e:
        with G.guarded(ops, poison) as g:
            allocate_like_ops(ops, (4, 4))
            v = allocate_like_ops(ops, (3, 5))
            a = g.allocations[1]
            assert a.view is v
            at = G.GUARD - 4 if side == "before" else G.GUARD + a.nbytes
            a.base[at:at + 4].view(torch.float32)[0] = 1.0       # through the base buffer: one float outside the view
    msg = str(e.value)
    assert "#1 torch.empty([3, 5], float32), 60 bytes" in msg and "#0" not in msg
    assert ("%s the view" % side) in msg and "allocate_like_ops:" in msg
    # 1.0f = 00 00 80 3F: all four bytes differ from either poison, the first damaged one is the float's first
    assert ("offset %+d from its %s" % ((-4, "start") if side == "before" else (0, "end"))) in msg
    assert ops.torch is torch and not isinstance(ops.lib, G.LibProxy)


def test_a_single_damaged_byte_deep_in_a_guard_is_found():
    ops = fake_ops()
    with G.guarded(ops, 0x7F, check=False) as g:
        allocate_like_ops(ops, (2,), torch.int64)
    g.check()
    g.allocations[0].base[-1] = 0
    (a, side, at), = g.damage()
    assert (side, at) == ("after", G.GUARD - 1)
    g.allocations[0].base[-1] = 0x7F
    g.allocations[0].base[0] = 0
    (a, side, at), = g.damage()
    assert (side, at) == ("before", -G.GUARD)


def test_an_exception_inside_the_block_is_not_replaced_by_the_guard_check():
    ops = fake_ops()
    with pytest.raises(KeyError):
        with G.guarded(ops, 0xFF) as g:
            allocate_like_ops(ops, (2,))
            g.allocations[0].base[0] = 0
            raise KeyError("the block's own failure")
    assert ops.torch is torch


def test_poison_shows_through_an_unwritten_view():
    ops = fake_ops()
    with G.guarded(ops, G.POISON_NAN) as g:
        f = allocate_like_ops(ops, (2, 3))
        i32 = allocate_like_ops(ops, (4,), torch.int32)
        i64 = allocate_like_ops(ops, (2, 2), torch.int64)
        u8 = allocate_like_ops(ops, 5, torch.uint8)
    assert torch.isnan(f).all() and (i32 == -1).all() and (i64 == -1).all() and (u8 == 255).all()
    assert i64.dtype == torch.int64 and tuple(i64.shape) == (2, 2) and tuple(u8.shape) == (5,)
    with G.guarded(ops, G.POISON_FINITE):
        f = allocate_like_ops(ops, (2, 3))
    assert torch.isfinite(f).all() and math.isclose(float(f[0, 0]), 3.3962e38, rel_tol=1e-4)
    assert not G.bit_equal(f, torch.zeros(2, 3)) and G.bit_equal(f, f.clone())


def test_zero_size_zeros_and_the_call_forms_ops_uses():
    ops = fake_ops()
    like = torch.ones(3, 2, dtype=torch.int32)
    with G.guarded(ops, 0xFF) as g:
        e0 = allocate_like_ops(ops, (0, 7))
        z = allocate_like_ops(ops, (3, 4), call="zeros")
        zl = ops.torch.zeros_like(like)
        el = ops.torch.empty_like(like)
        star = ops.torch.empty(2, 3, dtype=torch.float32, device="cpu")
        one = ops.torch.zeros(1, dtype=torch.int32, device="cpu")
        assert ops.torch.float32 is torch.float32 and ops.torch.cuda is torch.cuda     # everything else is forwarded
        assert isinstance(z, ops.torch.Tensor)
    assert tuple(e0.shape) == (0, 7) and e0.numel() == 0 and g.allocations[0].nbytes == 0
    assert tuple(z.shape) == (3, 4) and not z.any() and not zl.any() and zl.dtype == torch.int32
    assert tuple(el.shape) == (3, 2) and (el == -1).all() and tuple(star.shape) == (2, 3) and int(one) == 0
    z_rec = g.allocations[1]
    assert (z_rec.base[:G.GUARD] == 0xFF).all() and (z_rec.base[G.GUARD + z_rec.nbytes:] == 0xFF).all()
    with pytest.raises(TypeError):                         # a form the seam does not serve must not pass unguarded
        with G.guarded(ops, 0xFF):
            ops.torch.empty((2,), dtype=torch.float32, device="cpu", pin_memory=False)


def test_short_views_make_a_correct_writer_trip_the_guard():
    ops = fake_ops()
    for short_if, hit in ((None, True), (lambda a: a.frames[0].startswith("allocate_like_ops"), True),
                          (lambda a: False, False)):
        with G.guarded(ops, 0xFF, short_by=16, short_if=short_if, check=False) as g:
            allocate_like_ops(ops, (8,)).fill_(2.0)       # writes its 32 bytes and nothing else
            allocate_like_ops(ops, (8,))[:4] = 2.0        # leaves the last 16 bytes alone
        found = g.damage()
        assert [(a.index, side, at) for a, side, at in found] == ([(0, "after", -16)] if hit else [])


def test_the_lib_proxy_lists_the_workspace_queries():
    ops = fake_ops()
    with G.guarded(ops, 0xFF) as g:
        assert ops.lib.rec_mmoe_workspace_bytes(1, 2) == 64 and ops.lib.rec_mmoe_bwd_f32() == 0
        assert getattr(ops.lib, "rec_mmoe_workspace_bytes")() == 64
        with pytest.raises(AttributeError):
            ops.lib.rec_nothing_workspace_bytes
    assert g.queries == ["rec_mmoe_workspace_bytes"]


# ---- the text of ops.py ----------------------------------------------------------------------------------------------
def ops_text():
    with open(OPS_PATH) as f:
        return f.read()


def test_ops_allocates_only_through_the_four_calls_and_the_one_global():
    text = ops_text()
    assert re.findall(r"^import torch$", text, flags=re.M) == ["import torch"]
    assert not re.search(r"import torch\.|from torch|import torch as|^\s*import .*,\s*torch", text, flags=re.M)
    # no alias of the module or of a function of it: `t = torch`, `empty = torch.empty`, `getattr(torch, ...)`
    assert not re.search(r"=\s*torch\s*$|=\s*torch\.(empty|zeros|ones|full|tensor|arange)\w*\s*$|getattr\(torch\b|"
                         r"\(torch\)|,\s*torch\s*[,)]", text, flags=re.M)
    makers = ("empty", "empty_like", "empty_strided", "zeros", "zeros_like", "ones", "ones_like", "full", "full_like",
              "tensor", "as_tensor", "arange", "linspace", "eye", "rand", "randn", "randint", "from_numpy", "clone",
              "cat", "stack", "empty_permuted")
    used = set(re.findall(r"\btorch\.(%s)\b" % "|".join(makers), text))
    assert used == set(G.ALLOCATORS), used
    # tensor methods that allocate behind the seam's back
    assert not re.search(r"\.(new_empty|new_zeros|new_ones|new_full|new_tensor|clone)\(", text)


def test_every_workspace_query_of_ops_has_a_driver():
    from tests import test_gpu_guarded as T
    in_ops = set(G.QUERY.findall(ops_text()))
    declared = set().union(*(set(d.queries) for d in T.DRIVERS))
    print("workspace queries covered by a driver: %d of %d" % (len(in_ops & declared), len(in_ops)))
    assert len(in_ops) >= 22                               # 22 distinct names when this was written
    assert declared == in_ops, (sorted(in_ops - declared), sorted(declared - in_ops))
    assert all(d.cases for d in T.DRIVERS)
