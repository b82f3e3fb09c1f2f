"""CPU: where the pipeline picks the twin form of the two-sequence forward (pipeline.MotionDiffusion._session_opts) -- with the
session option `seq_twin` off, the (seq_pairs, seq_duo) of every role are the parent rule's; with it on (the default) only
the sessions for which that rule gives two sequences of a kind per workgroup, classifier-free pairs in workgroups of their own,
change -- and the argument block's new field."""
import types

import pytest


def _pipeline(rg, batch_lanes=4, cob=True, **session_options):
    MD = rg.pipeline.MotionDiffusion
    m = MD.__new__(MD)
    m.session_options, m.tail_glue = dict(session_options), True
    m.async_results, m.batch_lanes, m._cur_rot = True, batch_lanes, None
    m._cob = dict(lane=3) if cob else None
    m.invert_alone_wide = True
    m.model = types.SimpleNamespace(weights=types.SimpleNamespace(seq_streams=object()))
    m._seq_form_auto = lambda B: MD._seq_form_auto(m, B, cus=256)      # (a 256-CU device, without asking one)
    return m


def _forms(m, B, role):
    o = m._session_opts(B, role, 0)
    return bool(o["seq_pairs"]), bool(o["seq_duo"]), bool(o["seq_twin"])


CASES = [(4, 64, "cobatch"), (4, 48, "cobatch"), (4, 16, "sample"), (4, 32, "sample"), (4, 48, "invert"), (8, 64, "cobatch"),
         (8, 48, "invert"), (8, 32, "sample"), (8, 16, "sample"), (2, 64, "cobatch"), (2, 96, "cobatch")]


@pytest.mark.parametrize("lanes,B,role", CASES)
def test_option_off_gives_the_parent_forms(rg, lanes, B, role):
    m = _pipeline(rg, lanes, seq_twin=False)
    pairs, duo = m._seq_form_auto(B)
    if role == "invert":                      # an inversion alone: one workgroup per sequence (invert_alone_wide)
        pairs, duo = False, False
    assert _forms(m, B, role) == (pairs, duo, False)
    assert rg.pipeline.MotionDiffusion._form_tag(m._session_opts(B, role, 0)) == (pairs, duo, False)


@pytest.mark.parametrize("lanes,B,role", CASES)
def test_option_on_changes_only_the_duo_sessions(rg, lanes, B, role):
    off, on = _forms(_pipeline(rg, lanes, seq_twin=False), B, role), _forms(_pipeline(rg, lanes), B, role)
    assert on[:2] == off[:2]                                     # what bench.py and the other tests read stays
    assert on[2] == (off[:2] == (False, True))
    assert _forms(_pipeline(rg, lanes, seq_twin=True), B, role) == on


def test_twin_form_where_the_flagship_runs(rg):
    """Four lanes: the co-batched chains of 64 clips (16 + 48 exemplars) take the twin form, a draining batch and an inversion
    alone keep one workgroup per sequence; eight lanes keep the pairs form; synchronous forwards keep one per sequence."""
    m = _pipeline(rg)
    assert _forms(m, 64, "cobatch") == (False, True, True)
    assert _forms(m, 16, "sample") == (False, False, False) and _forms(m, 48, "invert") == (False, False, False)
    m.invert_alone_wide = False
    assert _forms(m, 48, "invert") == (False, True, True)
    assert _forms(_pipeline(rg, 8), 64, "cobatch") == (True, True, False)
    assert _forms(_pipeline(rg, 8), 48, "invert") == (False, False, False)
    m8 = _pipeline(rg, 8)
    m8.invert_alone_wide = False             # the pairs form widened for an inversion alone: left as it is
    assert _forms(m8, 48, "invert") == (False, True, False)
    assert _forms(_pipeline(rg, cob=False), 64, "sample") == (False, False, False)
    # explicit forms are the caller's word, with and without the option
    assert _forms(_pipeline(rg, seq_pairs=True, seq_duo=True), 64, "cobatch") == (True, True, False)
    assert _forms(_pipeline(rg, seq_pairs=False, seq_duo=True), 64, "cobatch") == (False, True, False)
    assert _forms(_pipeline(rg, seq_pairs=False, seq_duo=True, seq_twin=True), 64, "cobatch") == (False, True, True)
    # the form is part of a session's key
    tag = rg.pipeline.MotionDiffusion._form_tag
    assert tag(_pipeline(rg)._session_opts(64, "cobatch", 0)) != tag(_pipeline(rg, seq_twin=False)._session_opts(64, "cobatch", 0))


def test_argument_block_has_the_field(rg):
    a = rg.seqfwd.SeqArgs()
    assert a.twin == 0 and a.pairs == 0
    names = [f[0] for f in rg.seqfwd.SeqArgs._fields_]
    assert names.index("twin") == names.index("pairs") + 1 and names.index("glue_ctr") == names.index("twin") + 1
    assert rg.capi.header_version() >= 120
