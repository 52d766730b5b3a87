"""shared by the emulator and GPU tests of the deterministic mode: `SSS_ROWS_ORDERED_ADD` (include/sss.h; csrc/sss_rows.h)
against an in-order host sum, and the sort plans of spark_sched_sim_amd.train_kernels"""
import numpy as np
import torch

WIDTHS = (1, 2, 5, 16, 21, 36, 64)


def run_keys(rng, n: int, rows: int, max_run: int = 2000) -> np.ndarray:
    """i64[n] non-decreasing table rows < `rows`: runs of 1 .. max_run equal keys (both ends present when n allows), rows
    between the runs skipped at random"""
    lengths = []
    left = n
    if n >= max_run:
        lengths.append(max_run)
        left -= max_run
    if left > 0:
        lengths.append(1)
        left -= 1
    while left > 0:
        ln = int(min(left, rng.choice([1, 1, 2, 3, 5, 8, 40, 300]) if rng.random() < 0.95 else rng.integers(1, max_run + 1)))
        lengths.append(ln)
        left -= ln
    rng.shuffle(lengths)
    assert len(lengths) <= rows
    starts = np.sort(rng.choice(rows, size=len(lengths), replace=False))
    return np.repeat(starts, lengths).astype(np.int64)


def order_sensitive(rng, shape) -> np.ndarray:
    """float32 values whose sum depends on the order of the additions: +-1e8 next to values of order 10 (below the big ones' ulp
    of 8, they are rounded differently depending on what they are added to)"""
    big = rng.choice(np.array([-1e8, 1e8, 3e7, -3e7], dtype=np.float32), size=shape)
    small = rng.standard_normal(shape).astype(np.float32) * np.float32(40.0)
    return np.where(rng.random(shape) < 0.3, big, small).astype(np.float32)


def reference(b: np.ndarray, keys: np.ndarray, a: np.ndarray, perm) -> np.ndarray:
    """b[keys[k]] += a[p(k)] for k = 0, 1, ... in that order (np.add.at is unbuffered and adds in index order)"""
    out = b.copy()
    np.add.at(out, keys, a[perm] if perm is not None else a)
    return out


def check_ordered_add(binding, device, n: int, seed: int = 3):
    """ROWS_ORDERED_ADD bit for bit against `reference`: every width of WIDTHS, a whole list and a column slice of a wider matrix,
    perm NULL and a permutation, runs of 1 .. 2000 rows, a single run, n = 0. Returns the outputs of the column-slice form
    (by width and perm) for callers that compare forms."""
    from spark_sched_sim_amd.train_kernels import ROWS_ORDERED_ADD, rows_op

    rng = np.random.default_rng(seed)
    rows = max(64, n // 2)
    T = lambda x: torch.from_numpy(np.array(x, copy=True)).to(device)  # noqa: E731  (a copy: on the CPU the tensor would share b's memory)
    got_forms = {}
    for width in WIDTHS:
        keys = run_keys(rng, n, rows)
        assert (np.diff(keys) >= 0).all()
        runs = np.unique(keys, return_counts=True)[1]
        assert runs.min() == 1 and runs.max() == min(n, 2000)
        a = order_sensitive(rng, (n, width))
        b = order_sensitive(rng, (rows, width))
        perm = rng.permutation(n).astype(np.int64)
        # the check is only worth something if the order matters for the data: reversing every run changes many rows
        fwd = reference(b, keys, a, perm)
        back = reference(b, keys[::-1].copy(), a, perm[::-1].copy())
        assert int((fwd.view(np.uint32) != back.view(np.uint32)).any(1).sum()) >= max(3, int((runs >= 2).sum()) // 2), width
        wide = order_sensitive(rng, (n, width + 7))
        wide[:, 3:3 + width] = a
        wide_t = T(wide)
        for p in (None, perm):
            want = reference(b, keys, a, p)
            for form, a_t in (("whole", T(a)), ("slice", wide_t[:, 3:3 + width])):
                tab = T(b)
                rows_op(ROWS_ORDERED_ADD, T(keys), a_t, tab, binding=binding, perm=T(p) if p is not None else None)
                out = tab.cpu().numpy()
                bad = (out.view(np.uint32) != want.view(np.uint32)).any(1)
                assert not bad.any(), (width, form, p is None, int(bad.sum()), np.nonzero(bad)[0][:5])
                got_forms[(width, p is None, form)] = tab
        assert torch.equal(wide_t.cpu(), torch.from_numpy(wide))  # (the list side is read only)
    # one run over the whole list, and nothing at all
    a = order_sensitive(rng, (n, 16))
    b = order_sensitive(rng, (4, 16))
    keys = np.full(n, 2, dtype=np.int64)
    perm = rng.permutation(n).astype(np.int64)
    tab = T(b)
    rows_op(ROWS_ORDERED_ADD, T(keys), T(a), tab, binding=binding, perm=T(perm))
    assert np.array_equal(tab.cpu().numpy().view(np.uint32), reference(b, keys, a, perm).view(np.uint32))
    tab = T(b)
    rows_op(ROWS_ORDERED_ADD, torch.zeros(0, dtype=torch.int64, device=device), torch.zeros((0, 16), device=device), tab, binding=binding)
    assert torch.equal(tab.cpu(), torch.from_numpy(b))
    return got_forms


def check_rejected_ops(binding, device):
    """op 6 is an operation now; every other id above 5 is still refused"""
    import pytest

    from spark_sched_sim_amd.train_kernels import rows_op

    for op in (7, 8, 100, -1):
        with pytest.raises(ValueError):
            rows_op(op, torch.zeros(2, dtype=torch.long, device=device), torch.zeros((2, 16), device=device), torch.zeros((4, 16), device=device), binding=binding)


def check_plans(device):
    """`sort_plan`: keys = idx[perm] non-decreasing, perm ascending inside every run (a stable sort); `layer_plans`: the same per
    layer from one sort, positions counted inside the layer's list"""
    from spark_sched_sim_amd.train_kernels import layer_plans, sort_plan

    gen = torch.Generator().manual_seed(4)
    for n, rows in ((1, 1), (37, 5), (5000, 300), (20000, 19000)):
        idx = torch.randint(0, rows, (n,), generator=gen).to(device)
        keys, perm = sort_plan(idx)
        assert keys.dtype == perm.dtype == torch.int64
        assert bool((keys[1:] >= keys[:-1]).all()) and torch.equal(keys, idx[perm])
        assert torch.equal(torch.sort(perm)[0], torch.arange(n, device=device))
        same = keys[1:] == keys[:-1]
        assert bool((perm[1:][same] > perm[:-1][same]).all())
    M = 700
    children = [torch.randint(0, M, (k,), generator=gen).to(device) for k in (50, 0, 1, 900, 33)]
    plans = layer_plans(children, M)
    assert len(plans) == len(children)
    for c, (keys, perm) in zip(children, plans):
        k1, p1 = sort_plan(c)
        assert torch.equal(keys, k1) and torch.equal(perm, p1)
    assert [tuple(p[0].shape) for p in layer_plans(children[1:2], M)] == [(0,)]
