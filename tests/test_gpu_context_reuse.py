"""One context, many calls of changing size: a serving process keeps a context for days and sends
frames and match sets of every size through it, while most of the suite makes a fresh context per
call.  A context's buffers grow only and are never cleared (csrc/fm3d_ctx.h), so a stage is right
only if every call writes all that it or a later kernel reads, whatever the larger call before it
left behind: flags past n, list tails, an odd last row pair, pads, count words.

Every case of reuse_cases.py's table runs its sequence -- large, small, another stride or none at
all, large again -- on one context.  Every step equals the oracle or restatement its entry point's
own test compares with (the pipeline and the multi-GPU run: a fresh context's bytes, the small pair
the oracle too), and the first and last steps, which have the same input, are byte-equal."""
import pytest

import reuse_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", rc.CASES, ids=[c.name for c in rc.CASES])
def test_sequence_on_one_context(fm3d, orc, synth, case):
    world = rc.world(fm3d, orc, synth)
    assert case.steps[0] == case.steps[-1] and len(set(case.steps)) >= 2
    ctx = rc.open_ctx(fm3d, case, world)
    try:
        results = [rc.run_on(case, world, ctx, x) for x in case.steps]
    finally:
        ctx.close()
    for i, (x, got) in enumerate(zip(case.steps, results)):
        try:
            rc.check_reference(case, world, x, got)
        except AssertionError as e:
            raise AssertionError(f"{case.name}: step {i} ({x}) of {case.steps} differs from its reference: {e}") from e
    rc.assert_same(results[-1], results[0], f"{case.name}: last step vs first step ({case.steps[0]})")
