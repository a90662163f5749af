"""The native train step with the row-liveness mask on equals the step with it
off (Trainer.live_mask; nerf/native_step.py).

The field backward marks the field rows whose incoming gradient is exactly
zero (the samples past a ray's T < 1e-4 break) and the binned embedding
backward files none of them.  Such a row added w * 0 before, so nothing may
change: twin trainers at 32 x 32 from the same seed (bench.py's trainer: the
default Gaussian density blob, which is opaque enough at the centre for the
central rays to break from the first step, so nothing was raised), 20
graph-replayed steps crossing a density refresh, albedo and textureless with
the row-wise bin of the 7 M rows (Trainer.stencil_bin off), give equal loss,
parameters, Adam moments, scaler state, step counters and density grid.  The
default textureless step bins stencil groups, which take no mask: there the
switch must change nothing at all.

Against a vacuous pass, the dead-row share of the last step — counted from the
step's own gradient buffers, and from its mask — must lie in [0.02, 0.98].
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 20  # crosses a density-grid refresh


def _dead_share(nat):
    m = int(nat.m_field[0])
    gs, ga = nat.grad_sigma_field[:m], nat.grad_albedo[:m]
    dead = int(((gs == 0) & (ga == 0).all(dim=1)).sum())
    by_mask = None
    if nat.live_mask:
        words = nat.row_live[:(m + 31) // 32].cpu().numpy().view(np.uint32)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        assert not bits[m:].any()          # zero from the live count to the end of its word
        by_mask = m - int(bits[:m].sum())
    return m, dead, by_mask


@pytest.mark.parametrize("shade,stencil_bin", [("albedo", True), ("textureless", True),
                                               ("textureless", False)],
                         ids=["albedo", "textureless", "textureless-rowwise"])
def test_live_mask_on_equals_off(gpu, shade, stencil_bin):
    import bench

    def run(on):
        tr, dt = bench.make_trainer(32, 5, 0, 1, True, graph=True)
        tr.opt.iters = 50
        assert tr.live_mask is True  # default on
        tr.live_mask = on
        tr.stencil_bin = stencil_bin
        if shade != "albedo":
            tr.pick_shading = lambda: (shade, 0.1)
        for i in range(STEPS):
            tr.train_iteration(dt.collate([i % 4]))
        torch.cuda.synchronize()
        return tr
    a, b = run(True), run(False)
    ga, gb = next(iter(a._graphs.values())), next(iter(b._graphs.values()))
    na, nb = ga.native, gb.native
    assert na is not None and nb is not None and ga.optimizer_in_graph and gb.optimizer_in_graph
    # (stencil groups take no mask: the default textureless step runs without one)
    assert na.live_mask == (not na.stencil_bin) and not nb.live_mask
    assert na.shading == shade and na.stencil_bin == (stencil_bin and shade != "albedo")
    m, dead, by_mask = _dead_share(na)
    assert _dead_share(nb)[:2] == (m, dead)
    assert by_mask == (dead if na.live_mask else None)
    assert 0.02 <= dead / m <= 0.98, f"dead-row share {dead / m:.4f} of {m} rows"
    assert torch.equal(ga.loss, gb.loss)
    for pa, pb in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(pa, pb)
    assert torch.equal(a.model.encoder.embeddings.grad, b.model.encoder.embeddings.grad)
    sa, sb = a.optimizer.state_dict()["state"], b.optimizer.state_dict()["state"]
    for i in sa:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[i][name], sb[i][name]), (i, name)
    assert float(a.scaler.get_scale()) == float(b.scaler.get_scale())
    assert int(a.scaler._growth_tracker) == int(b.scaler._growth_tracker)
    assert torch.equal(a.model.step_counter, b.model.step_counter)
    assert torch.equal(a.model.density_grid, b.model.density_grid)
    assert torch.equal(a.model.density_bitfield, b.model.density_bitfield)
