"""GPU pin of the rasteriser's backward (grad_kernel.h, K5), element by element, against the float64 statement
(tests/backward_f64.py) under the derived bound of tests/backward_cases.py (its docstring carries the derivation;
DESIGN.md 5):

    |got - f64| <= (n - 1 + k) 2^-24 S,  exactly 0 where S == 0,   k_v = C + 15 (+ 3 clipped),  k_c = 14 (+ 3 clipped),

S the sum of the absolute values of the element's terms and n their number, plus 4 * 2^-24 N in the w component for
x_ndc's own rounding.  No oracle value takes part in a comparison: the oracle supplies the g-buffer the statement
needs, and the GPU's g-buffer is asserted equal to it.  Every case prints its worst error / bound ratio (and the
worst error in units of 2^-24 S); run with -s to see them.  Measured on an MI355X: DESIGN.md 5.

The whole table runs through the public path (rasterise_ops._rasterise_batched + autograd); three cases (plain,
clipped, slot-table overflow) also run through the kernel's other entries: the gradient subsets (GM = 1, 2),
dirt_rasterise_bwd_recompute with and without dirt_rasterise_fwd_stash, and the accumulate flag.
"""
import numpy as np
import pytest
import torch

import backward_cases as bc
from test_gpu_parity import _gpu, run_gpu

pytestmark = pytest.mark.gpu

ENTRY_CASES = ["frame_33x17", "fuzz_167059", "slot_overflow_c3"]  # plain, clipped (batch of two), slot overflow


def _dev(a):
    return _gpu(np.array(a))  # (a writable copy: the reference's arrays are read-only)


def _report(name, ratios):
    print("\n" + bc.fmt(name, ratios))


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_public_path_within_the_bound(name):
    ref = bc.reference(name)
    g = run_gpu(*(np.array(a) for a in ref.inputs), np.array(ref.gp))
    np.testing.assert_array_equal(g["gbuffer"], ref.gb)
    bc.check_background(g["grad_background"], ref)
    assert np.all(g["grad_vertices"][..., 2] == 0.0)
    _report(name, bc.check_bound(g["grad_vertices"], g["grad_colors"], ref))


def _session(ref):
    from dirt_amd.session import RasteriseSession
    bg, v, c, f = ref.inputs
    B, H, W, C = bg.shape
    sess = RasteriseSession(B, H, W, C, v.shape[1], f.shape[1], device="cuda")
    t = [_dev(a) for a in ref.inputs]
    sess.forward(*t)
    np.testing.assert_array_equal(sess.gbuffer.cpu().numpy(), ref.gb)
    return sess, t, (B, H, W, C, v.shape[1], f.shape[1])


def _bwd(sess, t, dims, gp, gv, gc, flags=0):
    from dirt_amd import _lib
    B, H, W, C, V, F = dims
    gbg = torch.empty((B, H, W, C), device="cuda")
    _lib.check(_lib.load().dirt_rasterise_bwd(
        t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), sess.pixels.data_ptr(), gp.data_ptr(),
        sess.gbuffer.data_ptr(), sess.saved.data_ptr(), B, H, W, C, V, F, gv.data_ptr() if gv is not None else None,
        gc.data_ptr() if gc is not None else None, gbg.data_ptr(), flags, torch.cuda.current_stream().cuda_stream))
    return gbg.cpu().numpy()


@pytest.mark.parametrize("name", ENTRY_CASES)
def test_gradient_subsets_within_the_bound(name):
    """Vertices only and colours only (the kernel's GM = 1 and GM = 2 instantiations)."""
    ref = bc.reference(name)
    sess, t, dims = _session(ref)
    B, H, W, C, V, F = dims
    gp = _dev(ref.gp)
    for want_v in (True, False):
        gv = torch.full((B, V, 4), 7.0, device="cuda") if want_v else None
        gc = None if want_v else torch.full((B, V, C), 7.0, device="cuda")
        bc.check_background(_bwd(sess, t, dims, gp, gv, gc), ref)
        _report(name + (" vertices only" if want_v else " colours only"),
                bc.check_bound(gv.cpu().numpy() if want_v else None, None if want_v else gc.cpu().numpy(), ref))


@pytest.mark.parametrize("stash", [False, True], ids=["miss", "stash"])
@pytest.mark.parametrize("name", ENTRY_CASES)
def test_recompute_backward_within_the_bound(name, stash):
    """dirt_rasterise_bwd_recompute on an empty workspace (it recomputes the forward's records) and on one that
    dirt_rasterise_fwd_stash filled (it reuses them)."""
    from dirt_amd import _lib
    lib = _lib.load()
    ref = bc.reference(name)
    bg, v, c, f = ref.inputs
    B, H, W, C = bg.shape
    V, F = v.shape[1], f.shape[1]
    t = [_dev(a) for a in ref.inputs]
    n = _lib.recompute_workspace_size(B, H, W, C, V, F)
    ws = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    px = _dev(ref.px)
    if stash:
        px = torch.empty((B, H, W, C), device="cuda")
        _lib.check(lib.dirt_rasterise_fwd_stash(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), B, H,
                                                W, C, V, F, px.data_ptr(), ws.data_ptr(), n, _lib.FWD_SCRATCH_CLEAN,
                                                stream))
        np.testing.assert_array_equal(px.cpu().numpy(), ref.px)
    gp = _dev(ref.gp)
    gv, gc = torch.full((B, V, 4), 7.0, device="cuda"), torch.full((B, V, C), 7.0, device="cuda")
    gbg = torch.empty((B, H, W, C), device="cuda")
    _lib.check(lib.dirt_rasterise_bwd_recompute(*(x.data_ptr() for x in t), px.data_ptr(), gp.data_ptr(), B, H, W, C, V,
                                                F, gv.data_ptr(), gc.data_ptr(), gbg.data_ptr(), ws.data_ptr(), n,
                                                _lib.BWD_SCRATCH_CLEAN, stream))
    assert _lib.stash_state(B, H, W, C, V, F, ws.data_ptr(), n, stream)["last_missed"] == (0 if stash else 1)
    bc.check_background(gbg.cpu().numpy(), ref)
    _report(name + (" recompute, stash" if stash else " recompute, miss"),
            bc.check_bound(gv.cpu().numpy(), gc.cpu().numpy(), ref))


@pytest.mark.parametrize("name", ENTRY_CASES)
def test_accumulate_flag_within_its_bound(name):
    """DIRT_BWD_ACCUMULATE adds into what the buffers hold; grad_background is overwritten.
      * A second backward on top of the first (what the flag is for): got - (held + f64) within the bound plus half
        an ulp of the held value (2^-24 |held| at most).
      * Held values that have nothing to do with the gradient (standard normal): every atomic add into an element
        rounds at the held value's ulp, not at the sum's, and an element receives up to n of them (one per tile and
        record, or per run tail), so the bound is (n + k) 2^-24 S + n 2^-24 |held|; with a single half ulp of the
        held value 4 of fuzz_167059's 750 elements reach 1.13 of the bound on an MI355X (|held| ~ 0.5 against
        S = 1e-3, two atomics).  Elements without terms keep the held value bit for bit."""
    from dirt_amd import _lib
    ref = bc.reference(name)
    sess, t, dims = _session(ref)
    B, H, W, C, V, F = dims
    gp = _dev(ref.gp)
    gv, gc = torch.full((B, V, 4), 7.0, device="cuda"), torch.full((B, V, C), 7.0, device="cuda")
    _bwd(sess, t, dims, gp, gv, gc)
    held_v, held_c = gv.cpu().numpy(), gc.cpu().numpy()
    bc.check_background(_bwd(sess, t, dims, gp, gv, gc, _lib.BWD_ACCUMULATE), ref)
    _report(name + " accumulate twice", bc.check_bound(
        gv.cpu().numpy(), gc.cpu().numpy(), ref, extra_v=bc.U * np.abs(held_v), extra_c=bc.U * np.abs(held_c),
        base_v=held_v.astype(np.float64), base_c=held_c.astype(np.float64)))
    rng = np.random.default_rng(11)
    held_v = rng.standard_normal((B, V, 4)).astype(np.float32)
    held_c = rng.standard_normal((B, V, C)).astype(np.float32)
    gv, gc = _gpu(held_v), _gpu(held_c)
    bc.check_background(_bwd(sess, t, dims, gp, gv, gc, _lib.BWD_ACCUMULATE), ref)
    got_v = gv.cpu().numpy()
    np.testing.assert_array_equal(got_v[..., 2], held_v[..., 2])
    _report(name + " accumulate onto noise", bc.check_bound(
        got_v, gc.cpu().numpy(), ref, extra_v=bc.U * (ref.n_v * np.abs(held_v) + ref.S_v),
        extra_c=bc.U * (ref.n_c * np.abs(held_c) + ref.S_c), base_v=held_v.astype(np.float64),
        base_c=held_c.astype(np.float64)))
