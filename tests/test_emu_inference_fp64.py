"""Decima's inference forward pass on the kernels (CPU wave emulator: the vector-unit forms) against the same forward pass in fp64 -
inference_fp64_util: every route of `DecimaPolicy` to an embedding or a score, tolerances from the fp32 tensor-op form's own error
against fp64 measured in the same run; the measured tables are in profiles/inference_fp64.md."""
import pytest

import inference_fp64_util as U
from decima_util import SCORE_ATOL
from emu_util import load_emu

DEV = "cpu"


@pytest.fixture(scope="module")
def prepared():
    """case -> (env, unbound policy, graph, fp64 forward pass, fp32 tensor-op forward pass), made once per case with the input conditions
    checked on the reference; the envs are closed with the module"""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = U.prepare(case, DEV, load_emu())
        return cache[case]
    yield get
    for env, *_ in cache.values():
        env.close()


@pytest.mark.parametrize("case", list(U.CASES))
def test_kernel_routes_match_the_fp64_forward_pass(prepared, case):
    """embeddings, job and observation summaries (relative to max(1, largest entry)), stage scores and executor scores (absolute, the
    -inf pattern equal) of every route within the bound of `inference_fp64_util.bounds_of` (`some_done`: plus its arithmetic terms); every route was the one it claims to be"""
    env, pol, g, ref, top = prepared(case)
    failures, rows = U.run_case(case, env, U.bind(pol, env), ref, top, g, U.arithmetic_terms("emu", case, pol, g, ref))
    print(f"{case}\n{U.table(rows)}")
    assert not failures, failures
    skipped = {r[0] for r in rows if r[4] is None}
    assert skipped == U.expected_skips(case, g, one_launch_kernel=False), skipped  # (the emulator has no matrix-core layers kernel)


@pytest.mark.parametrize("case", ["all_done", "all_done6"])
def test_a_graph_without_a_node_gives_no_action_on_every_route(prepared, case):
    """every env finished, no auto-reset: `act` on the exact-size graph (kernels bound, and tensor ops alone), `schedule_env` on the
    exact-size and on the capacity graph and `act_env` agree - no stage anywhere, the action `env.step` takes for "nothing to schedule"""
    env, pol, g, ref, top = prepared(case)
    U.check_no_node_routes(env, pol, ref)


@pytest.mark.parametrize("case", U.DECISION_CASES)
def test_greedy_decisions_are_the_fp64_arg_max(prepared, case):
    """`schedule_env(greedy=True)`, pipeline and one launch: stage and executor count equal the arg-max of the fp64 scores on every
    observation whose fp64 lead exceeds twice the case's bound; at most 5 % of the observations with a choice are such near-ties"""
    env, pol, g, ref, top = prepared(case)
    bound, _, failures = U.bounds_of(ref, top)
    assert not failures, failures
    n = U.check_decisions(env, U.bind(pol, env), g, ref, bound)
    print(case, n)


@pytest.mark.parametrize("case", ["small16", "one_env"])
@pytest.mark.parametrize("control", list(U.CONTROLS))
def test_the_comparison_fails_a_subtly_wrong_forward_pass(prepared, case, control):
    """negative controls: a Python entry point hands on a slightly wrong value (a bias entry of one weight image off by 1e-5, a child's
    message left out, a job's sum one node short, two feature columns swapped for the heads, the count feature one count on) -
    `compare` must report it. The first one stays under the 2e-5 of the older tests: they would not have seen it."""
    env, pol, g, ref, top = prepared(case)
    failures, rows = U.run_control(control, case, env, pol, g, ref, top)
    print(control, len(failures), failures[:3], U.worst(rows))
    assert failures
    if control == "update_image_last_bias_plus_1e-5":
        assert all(r[3] <= SCORE_ATOL for r in rows if r[4] is not None), U.worst(rows)
