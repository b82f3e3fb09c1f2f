"""CPU: the window decision of the grouped co-batched chains (pipeline.window_accepts, MotionDiffusion._twin_tail_form): pure
functions of what the parked chains and the new one are, in the manner of test_host_logic_cpu.py."""
import importlib
import types

P = importlib.import_module("rag-gesture_amd.pipeline")

SETT = (43, 50, True, (2,) * 50, 0.1)


def test_window_accepts():
    acc = P.window_accepts
    assert acc([], (0, SETT, 4), 4)
    assert acc([(0, SETT, 4)], (1, SETT, 4), 4) and acc([(0, SETT, 4), (1, SETT, 4), (3, SETT, 4)], (2, SETT, 4), 4)
    assert not acc([(0, SETT, 4)], (0, SETT, 4), 4)                                    # the lane already holds a parked chain
    assert not acc([(0, SETT, 4)], (1, SETT[:4] + (0.05,), 4), 4)                      # another guidance rate
    assert not acc([(0, SETT, 4)], (1, (27,) + SETT[1:], 4), 4)                        # another T
    assert not acc([(0, SETT, 4)], (1, SETT[:2] + (False,) + SETT[3:], 4), 4)          # plain sampling beside guided
    assert not acc([(0, SETT, 4)], (1, SETT, 2), 2)                                    # another rotation
    assert not acc([(0, SETT, 2), (1, SETT, 2)], (2, SETT, 2), 2)                      # the window is full
    assert not acc([(0, SETT, 4), (2, SETT[:4] + (0.05,), 4)], (1, SETT, 4), 4)        # every parked chain counts, not the first alone


def test_twin_tail_form():
    me = types.SimpleNamespace(_runs_seq_engine=lambda o: o.get("engine") != "chain")
    form = lambda **o: P.MotionDiffusion._twin_tail_form(me, o)
    twin = dict(seq_twin=True, seq_duo=True, seq_pairs=False, tail_glue=True)
    assert form(**twin)
    assert not form(**dict(twin, seq_twin=False)) and not form(**dict(twin, seq_duo=False)) and not form(**dict(twin, seq_pairs=True))
    assert not form(**dict(twin, tail_glue=False)) and not form(**dict(twin, engine="chain"))


def test_option_defaults():
    import inspect
    sig = inspect.signature(P.MotionDiffusion.__init__)
    assert sig.parameters["grouped_chains"].default is True and sig.parameters["grouped_drain"].default is True
    assert 2 <= P.MotionDiffusion.CHAIN_GROUP <= importlib.import_module("rag-gesture_amd.sampler").MANY_MAX
