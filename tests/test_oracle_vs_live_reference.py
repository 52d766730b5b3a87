"""The oracle and the kernel source against the REFERENCE ITSELF on trace-set regimes that neither committed fixture profile covers:
generator parameters / an env configuration / a policy drawn from a seed (tests/golden/make_golden.py random_regime: 2-30 stages,
in-degree 1-5 with near or far parents, 1-60 tasks per stage scaled by size, any subset of the executor levels, bases from 20 ms to
20 s, 3-128 executors, zero and non-zero delays; executor counts on both sides of the 64-lane boundary). One episode of each regime
was recorded from the reference the way the committed fixtures were (tests/golden/random_regime_<seed>.npz,
tests/golden/decima_random_<seed>.npz), and the C oracle (oracle/sss_oracle.c) and the kernel source under the CPU wave emulator
must reproduce it bit for bit. The recordings are regenerated where the reference is available:

    python tests/golden/make_golden.py --random SEED tests/golden/random_regime_SEED.npz
    python tests/golden/make_decima_golden.py --random SEED tests/golden/decima_random_SEED.npz
"""
import os.path as osp

import pytest

from golden_util import GOLDEN_DIR, Golden
from oracle_binding import OracleEnv


@pytest.mark.parametrize("seed", list(range(10)))
def test_oracle_and_kernel_source_match_the_live_reference_on_a_random_regime(seed):
    import test_oracle_golden as T
    from emu_util import load_emu
    from replay_util import replay_golden

    g = Golden("random", path=osp.join(GOLDEN_DIR, f"random_regime_{seed}.npz"))
    pack = g.pack(b"")
    s = g.seeds[0]
    # the oracle: every recorded step (rewards / wall times / digests / the first observations in full / job times)
    env = OracleEnv(pack, g.cfg)
    T.replay(env, g, s)
    env.close()
    # the kernel source under the emulator, through the C ABI: the same recording (a reference episode that ended in its own
    # "[step]" assertion is replayed up to that step)
    import golden_util
    keep = golden_util.Golden
    try:
        golden_util.Golden = lambda name: g   # (replay_golden looks its fixture up by name)
        import replay_util
        replay_util.Golden = golden_util.Golden
        bad = replay_golden("random", [s], pack, device="cpu", lib=load_emu(), full_obs_steps=10, max_steps=120)
    finally:
        golden_util.Golden = keep
        replay_util.Golden = keep
    assert not bad, "\n".join(bad[:8])


@pytest.mark.parametrize("seed", [1, 4, 8])
def test_decima_features_and_scores_match_the_live_reference_on_a_random_regime(seed):
    """the same for SURVEY 8(f) next-1: the reference's own DecimaEnvWrapper / DecimaScheduler (functional PyG stand-ins) recorded on a
    random regime; over 40 steps node features, masks, DAG-layer edge masks identical, scores within 2e-5, graph kernel == tensor-op graph"""
    from decima_util import check_decima_fixture
    from emu_util import load_emu

    check_decima_fixture("random", "cpu", load_emu(), 40, path=osp.join(GOLDEN_DIR, f"decima_random_{seed}.npz"))
