"""csrc/k_match.hip and csrc/assignment.h without a GPU: the kernels' own source compiled for the host with g++ behind a lockstep emulation of a workgroup
(tests/host_emul/) and held to the numpy restatement of include/kasf.h's two rules (tests/match_ref.py) bit for bit on every output of both kernels: at frame
counts around the 256-frame tile, at sample counts around the 16-sample chunk, with 1, 7, 17, 22 and 64 rows (one and several blocks of rows, a last block
that is not full), with and without weights, with a lens; the grouping on the pair costs of the synthetic scene and on planted matrices with exact ties and
BIG entries, with too few groups; canaries around every array, inputs unchanged, no LDS beyond what the launch asked for.  It shows the kernels' logic, their
indexing and their fp64 operation order; what only the device can show stays with tests/test_gpu_match.py."""
import ctypes as C

import numpy as np
import pytest

from tests.host_emul import build, vp
from tests.match_ref import BIG, groups_np, pair_costs_np, partition_of, same_bits, scene, truth_partition

GROUP_OUT = ("group", "members", "views", "group_cost", "count", "dropped")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "match_host", "emul_match.cpp")
    lib.emul_match_workspace.restype = C.c_int64
    lib.emul_match_pair_costs.restype = C.c_int
    lib.emul_match_groups.restype = C.c_int
    return lib


class Guarded:
    """An array of `shape` whose first element lies `offset` bytes past a multiple of 16, with 64 canary bytes on either side."""

    def __init__(self, shape, dtype, offset=0, data=None, fill=0):
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        self.buf = np.full(self.nbytes + 160, 0x5A, np.uint8)
        self.start = 64 + (-(self.buf.ctypes.data + 64) % 16) + offset
        self.a = self.buf[self.start:self.start + self.nbytes].view(dtype).reshape(shape)
        self.a[...] = fill if data is None else data
        self.keep = self.buf.copy()

    def unchanged(self):
        return np.array_equal(self.buf, self.keep)

    def intact(self):
        return np.array_equal(self.buf[:self.start], self.keep[:self.start]) and np.array_equal(self.buf[self.start + self.nbytes:], self.keep[self.start + self.nbytes:])


def run_costs(emul, K, cams, offset=0, **kw):
    views, P, N, J = K.shape[:4]
    q = dict(min_score=0.3, weighted=True, cap=50.0, min_samples=2 * J, undistort_iterations=5)
    q.update(kw)
    kin, cin = Guarded(K.shape, np.float32, offset, K), Guarded(cams.shape, np.float32, 0, cams)
    cost, samples = Guarded((views, views, P, P), np.float32, offset, fill=9.0), Guarded((views, views, P, P), np.int32, offset, fill=77)
    nbytes = emul.emul_match_workspace(views, P, C.c_int64(N))
    assert nbytes == 20 * ((N + 255) // 256) * (views * (views - 1) // 2) * P * P
    work = Guarded((max(nbytes, 8) // 4,), np.int32, 8, fill=-1)
    overrun = emul.emul_match_pair_costs(vp(kin.a), views, P, C.c_int64(N), J, vp(cin.a), C.c_float(q["min_score"]), int(q["weighted"]), C.c_float(q["cap"]),
                                         q["min_samples"], q["undistort_iterations"], vp(cost.a), vp(samples.a), vp(work.a))
    assert overrun == 0
    assert kin.unchanged() and cin.unchanged() and cost.intact() and samples.intact() and work.intact()
    return cost.a, samples.a


def run_groups(emul, cost, samples, max_cost=15.0, G=None):
    views, P = cost.shape[0], cost.shape[2]
    G = min(64, 2 * P) if G is None else G
    cin, sin = Guarded(cost.shape, np.float32, 4, cost), Guarded(samples.shape, np.int32, 0, samples)
    shapes = dict(group=(views, P), members=(G, views), views=(G,), group_cost=(G,), count=(1,), dropped=(1,))
    out = {k: Guarded(s, np.float32 if k == "group_cost" else np.int32, 4 if k in ("group", "members") else 0, fill=77) for k, s in shapes.items()}
    overrun = emul.emul_match_groups(vp(cin.a), vp(sin.a), views, P, C.c_float(max_cost), G, *[vp(out[k].a) for k in GROUP_OUT])
    assert overrun == 0
    assert cin.unchanged() and sin.unchanged() and all(o.intact() for o in out.values())
    return {k: out[k].a for k in GROUP_OUT}


def check_costs(got, want):
    for name, a, b in zip(("cost", "samples"), got, want):
        assert same_bits(a, b), (name, np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:6])


def check_groups(got, want):
    for k in GROUP_OUT:
        assert same_bits(got[k].reshape(np.shape(want[k])), np.ascontiguousarray(want[k])), (k, got[k], want[k])


def test_one_camera_pair_one_row_one_sample(emul):
    K, cams, _, _ = scene(frames=1, cameras=2, players=1, joints=1, pad=0, seed=1)
    want = pair_costs_np(K, cams, min_samples=1)
    assert want[1][0, 1, 0, 0] == 1 and np.isfinite(want[0][0, 1, 0, 0])
    check_costs(run_costs(emul, K, cams, min_samples=1), want)
    check_costs(run_costs(emul, K, cams), pair_costs_np(K, cams))       # min_samples = 2 J not reached: +inf with a sample
    assert np.isinf(pair_costs_np(K, cams)[0]).all()


@pytest.mark.parametrize("frames", [255, 256, 257])
@pytest.mark.parametrize("offset", [0, 4])
def test_frame_counts_around_the_tile(emul, frames, offset):
    K, cams, _, _ = scene(frames=frames, cameras=2, players=2, joints=3, pad=1, seed=frames, lifetimes=True)
    want = pair_costs_np(K, cams)
    assert np.isfinite(want[0]).sum() >= 8 and (want[1] == 0).any()
    check_costs(run_costs(emul, K, cams, offset), want)


@pytest.mark.parametrize("frames,joints", [(1, 15), (1, 16), (1, 17), (3, 11), (24, 17)])
def test_sample_counts_around_the_chunk_with_the_scene(emul, frames, joints):
    K, cams, _, _ = scene(frames=frames, cameras=3, players=5, joints=joints, pad=1, seed=joints, lifetimes=frames > 8)
    want = pair_costs_np(K, cams, min_samples=joints)
    assert np.isfinite(want[0]).any()
    check_costs(run_costs(emul, K, cams, min_samples=joints), want)


@pytest.mark.parametrize("rows", [17, 22, 64])
def test_several_blocks_of_rows(emul, rows):
    """17 rows: blocks of 15 and 2; 22: two of 11; 64: sixteen of 4, the LDS ceiling."""
    K, cams, _, _ = scene(frames=2, cameras=2, players=rows - 2, joints=3, pad=2, seed=rows)
    want = pair_costs_np(K, cams)
    assert np.isfinite(want[0]).sum() >= 2 * (rows - 4) ** 2
    check_costs(run_costs(emul, K, cams, 4), want)


@pytest.mark.parametrize("kw", [dict(weighted=False), dict(cap=5.0, min_score=0.7), dict(undistort_iterations=0), dict(undistort_iterations=1, min_samples=1)])
def test_other_parameters(emul, kw):
    K, cams, _, _ = scene(frames=5, cameras=3, players=5, joints=17, pad=1, seed=9)
    K[0, 0, 1, 2, 0] = np.nan
    K[1, 2, 3, 4, 1] = np.inf
    want = pair_costs_np(K, cams, **kw)
    check_costs(run_costs(emul, K, cams, **kw), want)
    assert not same_bits(want[0], pair_costs_np(K, cams)[0])


def test_a_camera_that_is_not_finite_and_cameras_with_one_centre(emul):
    K, cams, _, _ = scene(frames=4, cameras=4, players=3, joints=5, pad=0, seed=11)
    cams[3] = cams[0]                                                   # a second feed of camera 0: s = t = 0, never comparable
    cams[2, 13] = np.nan
    want = pair_costs_np(K, cams, min_samples=1)
    assert (want[1][0, 3] == 0).all() and (want[1][2] == 0).all() and (want[1][0, 1] > 0).any()
    check_costs(run_costs(emul, K, cams, min_samples=1), want)


def test_a_pair_alone_equals_the_pair_among_three_cameras(emul):
    K, cams, _, _ = scene(frames=9, cameras=3, players=4, joints=17, pad=1, seed=12)
    full = run_costs(emul, K, cams)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        two = run_costs(emul, K[[a, b]], cams[[a, b]])
        assert same_bits(two[0][0, 1], full[0][a, b]) and same_bits(two[1][0, 1], full[1][a, b]) and same_bits(two[0][1, 0], full[0][b, a])


def test_groups_of_the_scene(emul):
    K, cams, _, row = scene(frames=6, cameras=5, players=6, joints=17, pad=1, seed=0)
    cost, samples = pair_costs_np(K, cams)
    want = groups_np(cost, samples)
    assert partition_of(want["members"]) == truth_partition(row)
    check_groups(run_groups(emul, cost, samples), want)
    for G, max_cost in ((3, 15.0), (6, 1.0), (64, 1e6)):                # too few groups; nearly everything rejected; nearly everything accepted
        want = groups_np(cost, samples, max_cost, G)
        check_groups(run_groups(emul, cost, samples, max_cost, G), want)
    assert groups_np(cost, samples, 15.0, 3)["dropped"] > 0 and groups_np(cost, samples, 1.0, 6)["dropped"] > 0


def planted(views, P, seed):
    """Costs on a grid of quarter pixels, so that exact ties abound, pairs without samples (BIG for a group of such members) and +inf costs."""
    rng = np.random.default_rng(seed)
    cost = (rng.integers(0, 12, (views, views, P, P)) * 0.25).astype(np.float32)
    samples = rng.integers(1, 4, (views, views, P, P)).astype(np.int32) * 10
    samples[rng.random(samples.shape) < 0.3] = 0
    cost[rng.random(cost.shape) < 0.2] = np.inf
    for a in range(views):
        for b in range(a, views):
            cost[b, a], samples[b, a] = cost[a, b].T, samples[a, b].T
        cost[a, a], samples[a, a] = np.inf, 0
    samples[:, :, P - 1, :] = samples[:, :, :, P - 1] = 0               # the last row of every camera is empty
    return cost, samples


@pytest.mark.parametrize("views,P,G,max_cost", [(2, 1, 1, 15.0), (3, 5, 10, 2.0), (4, 9, 6, 1.5), (16, 8, 64, 1.0), (3, 64, 64, 2.0), (5, 33, 40, 0.5)])
def test_groups_on_planted_costs_with_ties_and_big_entries(emul, views, P, G, max_cost):
    cost, samples = planted(views, P, views * 100 + P)
    want = groups_np(cost, samples, max_cost, G)
    if P > 4:
        assert (want["group"][:, P - 1] == -1).all() and want["count"] > 1 and (want["views"] > 1).any()
    check_groups(run_groups(emul, cost, samples, max_cost, G), want)
    assert BIG > 1e6
