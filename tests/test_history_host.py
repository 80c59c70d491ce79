"""The inputs of tests/test_hip_history.py, checked without a GPU: every script stays inside the documented reproducibility
claims (no word id more than 64 times in a call), its geometries cross the kernel thresholds they are there for, and the two
evaluations of s7 meet the same news ids, so that a stale news-vector cache would be hit."""
import numpy as np
import pytest

from tests import history as hs
from tests.test_hip_history import CASES


def _calls(fam):
    """(name, batch dict or word-id array) of every call one script makes."""
    for step in fam.script():
        if step.kind == "evaluate":
            for i, b in enumerate(step.batch[0]):
                yield "%s batch %d" % (step.name, i), b
        elif step.kind != "load":
            yield step.name, step.batch
        if step.kind == "autograd":
            yield "s6 eval forward", fam.batch("s6e")
            for n in hs.S6_TITLES:
                yield "s6 %d titles" % n, {"titles": hs.titles(n, hs.GEOM["s6"][3], 77 + n)}
                if hasattr(fam, "news"):
                    arrays = fam.news(n, 77 + n)
                    yield "s6 %d news" % n, {"titles": arrays[0], "absts": arrays[1] if arrays[1].ndim == 2 else np.zeros((1, 1), np.int64)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_no_word_id_occurs_more_than_64_times_in_a_call(case):
    fam = CASES[case]()
    seen = 0
    for name, batch in _calls(fam):
        arrays = hs.word_id_arrays(batch)
        for a in arrays:
            assert a.dtype == np.int64 and a.min() >= 0 and a.max() < hs.N_WORDS, (case, name)
        n = hs.max_word_occurrences(*arrays) if arrays else 0
        assert n <= hs.MAX_OCCURRENCES, "%s %s: a word id occurs %d times" % (case, name, n)
        seen += len(arrays)
    assert seen > 0 or case.startswith("bert")          # nrms_bert reads news ids, no words


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_script_has_the_steps_the_family_supports(case):
    fam = CASES[case]()
    names = [s.name for s in fam.script()]
    want = ["s0", "s1", "s2", "s3"] + (["s3p"] if fam.has_pooled else []) + ["s4", "s5", "s6", "s7a", "s7b", "s7c"]
    want += ["s8a", "s8b", "s8c", "s8d"] if fam.has_pad_flag else []
    assert names == want
    assert fam.has_pooled == (not case.startswith(("hierec", "graph")))        # the two models that refuse the pooled loss
    assert fam.has_pad_flag == (not case.startswith("bert"))                   # no word table, no pad-row flag
    oracle = [s.name for s in fam.script() if s.extra.get("oracle")]
    assert oracle == [names[-1] if fam.has_pad_flag else "s7b"]                # the last training step of the script
    for s in fam.script():
        if s.kind in ("train", "pooled", "eval_forward", "autograd"):
            key = "browsed_ids" if case.startswith("bert") else "browsed_titles"
            geom = hs.GEOM[{"s7b": "s7", "s8b": "s8", "s8d": "s8"}.get(s.name, s.name)]
            assert s.batch[key].shape[:2] == geom[:2], (case, s.name)
            assert s.batch["candidate_mask"].shape == (geom[0], geom[2])
            if not case.startswith("bert"):
                assert s.batch["browsed_titles"].shape[2] == geom[3]
        if s.kind == "pooled":
            assert "candidate_ids" in s.batch and "browsed_ids" in s.batch
    if case.startswith("naml"):
        assert fam.script()[0].batch["browsed_absts"].shape[2] == hs.ABST_WORDS == 17


def test_geometries_cross_the_thresholds_they_are_there_for():
    G = hs.GEOM
    titles_of = lambda g: g[0] * (g[1] + g[2])
    # every later training buffer is an oversized reuse of s0's
    assert all(titles_of(G[s]) * G[s][3] <= titles_of(G["s0"]) * G["s0"][3] for s in ("s1", "s3", "s3p", "s4", "s5", "s6", "s7", "s8"))
    # the fp16 padding-token row (row M = titles * L of the x16 buffer) moves when the batch shrinks
    assert titles_of(G["s0"]) * G["s0"][3] == 9900 and titles_of(G["s1"]) * G["s1"][3] == 1650
    # history: 50 and 33 on the fused user-encoder kernel (32 < H <= 64), 32 on the chain / the 32-row kernels
    assert (G["s0"][1], G["s3"][1], G["s4"][1], G["s8"][1]) == (50, 33, 32, 32)
    # titles: 30 and 12 on the 32-row kernels, 33 on the 64-row ones
    assert (G["s0"][3], G["s3"][3], G["s4"][3]) == (30, 12, 33) and G["s3"][3] < 32 < G["s4"][3] <= 64
    assert G["s3p"] == G["s3"] and G["s5"] == G["s0"] == G["s6"]
    # s2: more candidates than any training step has (C = 24 against 5: 72 candidate slots against 30)
    assert G["s2"][2] == 24 and G["s2"][0] * G["s2"][2] > max(G[s][0] * G[s][2] for s in ("s0", "s1", "s3", "s4", "s5"))
    # s6: get_news_vector on fewer, then more titles than the training forward holds
    assert hs.S6_TITLES[0] < titles_of(G["s6"]) == 330 < hs.S6_TITLES[1] and hs.S6_TITLES == (40, 400)
    assert titles_of(G["s6e"]) < titles_of(G["s6"])            # the interleaved eval forward reuses the training-sized storage
    assert G["s8"] == (4, 32, 5, 12)
    assert hs.N_WORDS == 30000 and hs.MAX_OCCURRENCES == 64


def test_the_two_evaluations_of_s7_meet_the_same_news():
    batches, labels, cat = hs.eval_set()
    assert [len(b["browsed_ids"]) for b in batches] == list(hs.S7_BATCHES) == [8, 3]
    assert len(labels) == sum(hs.S7_BATCHES)
    ids = []
    for b in batches:
        assert b["candidate_ids"].shape[1] == hs.S7_C == 24 and b["browsed_ids"].shape[1] == 50
        assert b["browsed_ids"].max() < hs.N_NEWS and b["candidate_ids"].max() < hs.N_NEWS
        # a slot's title is its news item's title: the per-id cache is consistent with what a slot-by-slot pass encodes
        assert np.array_equal(b["browsed_titles"], cat[b["browsed_ids"]]) and np.array_equal(b["candidate_titles"], cat[b["candidate_ids"]])
        assert not cat[0].any() and (b["browsed_ids"][b["browsed_mask"] == 0] == 0).all()
        ids.append(np.unique(np.concatenate([b["browsed_ids"].ravel(), b["candidate_ids"].ravel()])))
    for y, n in zip(labels, np.concatenate([b["candidate_mask"].sum(1) for b in batches])):
        assert len(y) == n and 0 < sum(y) < len(y)
    # news shared between the batches of one evaluation: looked up, not encoded, the second time
    assert np.intersect1d(ids[0][ids[0] > 0], ids[1][ids[1] > 0]).size > 10
    # both evaluations of every family run on these very batches: every id of the second was cached by the first
    for case in sorted(CASES):
        ev = [s for s in CASES[case]().script() if s.kind == "evaluate"]
        assert len(ev) == 2 and ev[0].batch is ev[1].batch
        for b, ref in zip(ev[0].batch[0], batches):
            assert np.array_equal(b["browsed_ids"], ref["browsed_ids"]) and np.array_equal(b["candidate_ids"], ref["candidate_ids"])
