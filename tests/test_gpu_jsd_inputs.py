"""GPU checks of the occupancy-JSD front door: jensen_shannon_divergence with its two arguments on different devices or of a float
dtype, occupancy_grid's shape / dtype / device checks (ValueError before a pointer reaches the kernel), and the kernel's own branch
for points beyond 1e5 (a full scan of every column) against the float64 brute force."""
import numpy as np
import pytest
import torch

import _jsd_case as jc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ev():
    from difffacto_amd import build
    build.build(verbose=False)
    from difffacto_amd import evaluation
    return evaluation


def test_jsd_arguments_on_different_devices(ev):
    z = jc.load_case(28, True)
    a, b = z["counters_a"].astype(np.int64), z["counters_b"].astype(np.int64)
    want = float(z["jsd_ab"])
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    both = ev.jensen_shannon_divergence(da, db)
    for P, Q in ((da, torch.from_numpy(b)), (torch.from_numpy(a), db), (da, b), (a, db), (da, torch.from_numpy(b).int()),
                 (da.double(), torch.from_numpy(z["counters_b"])), (da.float(), db)):
        got = ev.jensen_shannon_divergence(P, Q)
        assert type(got).__name__ == "float64" and abs(got - want) < 1e-11, (got, want)
    assert ev.jensen_shannon_divergence(da, torch.from_numpy(b)) == both == ev.jensen_shannon_divergence(torch.from_numpy(a), db)
    assert ev.jensen_shannon_divergence(da, torch.from_numpy(a)) == 0.0
    # the example of a mixed call: a device counter row against recorded host counters
    x = jc.load_clouds()["a"]
    row = ev.occupancy_grid(x)[0][0]
    assert abs(ev.jensen_shannon_divergence(row, torch.from_numpy(b)) - want) < 1e-11


def test_jsd_of_device_float_weights_is_not_truncated(ev):
    rng = np.random.default_rng(11)
    P, Q = rng.uniform(0, 1, 500), rng.uniform(0, 1, 500)
    want = ev.jensen_shannon_divergence(P, Q)
    got = ev.jensen_shannon_divergence(torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda())
    assert np.isfinite(got) and abs(got - want) < 1e-11 and 0.0 < got <= 1.0


def test_jsd_value_errors_on_the_device(ev):
    p = torch.tensor([3, 1, 0, 2]).cuda()
    with pytest.raises(ValueError, match="Negative values"):
        ev.jensen_shannon_divergence(p, torch.tensor([1, -1, 0, 2]))
    with pytest.raises(ValueError, match="Non equal size"):
        ev.jensen_shannon_divergence(p, torch.tensor([1, 1, 2]))
    with pytest.raises(ValueError, match="Non equal size"):
        ev.jensen_shannon_divergence(p.reshape(2, 2), torch.tensor([[1, 1, 2], [1, 1, 2]]).cuda())   # equal len, unequal size


def test_occupancy_grid_checks_shapes_before_the_kernel(ev):
    x = torch.from_numpy(jc.load_clouds()["a"]).cuda()          # (6, 256, 3)
    B, N, _ = x.shape
    lab = torch.zeros(B, N, dtype=torch.int32).cuda()
    for kw in (dict(labels=lab[:, :-1], n_class=4), dict(labels=lab[:-1], n_class=4), dict(labels=lab.reshape(-1), n_class=4),
               dict(labels=lab, n_class=17), dict(labels=lab, n_class=-1)):
        with pytest.raises(ValueError, match="occupancy_grid"):
            ev.occupancy_grid(x, resolution=8, **kw)
    for bad in (x[..., :2], x[0], x[:, :0]):
        with pytest.raises(ValueError, match="occupancy_grid"):
            ev.occupancy_grid(bad, resolution=8)
    c, b, _, n_bad = ev.occupancy_grid(x, resolution=8)
    keep = c.clone()
    for out in ((c[:, :-1], b, n_bad), (c, b[:, :-1], n_bad), (c.int(), b, n_bad), (c, b.long(), n_bad), (c.cpu(), b, n_bad),
                (c, b, n_bad.cpu()), (c, b, torch.zeros(2, dtype=torch.int32).cuda()), (c, b, n_bad.long()), (c, b, 0)):
        with pytest.raises(ValueError, match="occupancy_grid"):
            ev.occupancy_grid(x, resolution=8, out=out)
    with pytest.raises(ValueError, match="occupancy_grid"):     # rows of a labelled call do not fit an unlabelled out
        ev.occupancy_grid(x, lab, 4, resolution=8, out=(c, b, n_bad))
    assert torch.equal(c, keep)                                  # a refused call adds nothing


@pytest.mark.parametrize("R,sphere,N", [(28, True, 65), (40, False, 63), (3, True, 65)])
def test_far_points_on_the_device(ev, R, sphere, N):
    """Coordinates beyond 1e5 take the kernel's full scan; 1e7 and 1e20 as in the host-compiled check, one axis or all three."""
    rng = np.random.default_rng(R + N)
    x = jc.mixed_points(rng, 2 * N).reshape(2, N, 3)
    d = rng.standard_normal((12, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = np.concatenate([1e7 * d[:4], 1e20 * d[4:8], 2e5 * d[8:]]).astype(np.float32)
    x[0, :12], x[1, 5:17] = far, far[::-1]
    x[1, 20] = (0.1, -3e5, 0.2)                                  # far along one axis only
    x[1, 21] = (1.0e5, 0.0, 0.0)                                 # the threshold itself: not far
    want = jc.brute_force(x, R, sphere).reshape(2, N)
    c, bern, i, bad = ev.occupancy_grid(torch.from_numpy(x).cuda(), resolution=R, in_sphere=sphere, return_index=True)
    assert int(bad) == 0 and np.array_equal(i.cpu().numpy(), want)
    wc, wb = jc.count(want, ev.occupancy_num_cells(R, sphere))
    assert np.array_equal(c.cpu().numpy(), wc) and np.array_equal(bern.cpu().numpy(), wb)
