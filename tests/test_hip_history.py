"""Engine results must not depend on the calls made before them (tests/history.py has the script, the twin and the poison).

One case per (model family, precision).  Each case runs the script on one long-lived model once per poison of guarded.POISONS;
every step is compared bit for bit with the same step on a fresh twin put into the same logical state from outside, and the last
training step of the script is also held to the family's float64 oracle at the tolerances of the family's own test file
(imported, not restated), so that two models agreeing on nothing-done cannot pass.

The script (geometry = users, history slots, candidates, words per title; training steps with dropout 0.2, new data per step):
  s0  train_step (6, 50, 5, 30)     largest first          s1  train_step (1, 50, 5, 30)   one user
  s2  eval forward (3, 50, 24, 30)  dedup on, then off     s3  train_step (5, 33, 3, 12)   H = 33, short titles
  s3p train_step, pooled loss (5, 33, 3, 12)               s4  train_step (4, 32, 5, 33)   H = 32, L = 33
  s5  train_step (6, 50, 5, 30)     the first shape again
  s6  autograd: model(batch), get_news_vector on 40 then 400 titles and an eval forward (3, 50, 24, 30) over the distinct titles
      and over every slot, loss.backward(); the twin runs forward and backward with nothing in between (and the inference calls
      afterwards, which must give the same bits too)
  s7  train_eval.evaluate (B = 8 and B = 3, C = 24, 300 news), train_step, evaluate again on the same batches
  s8  load_state_dict with a non-zero padding row, train_step (4, 32, 5, 12), the zero-row weights back, train_step

Steps a family lacks (named again in the family classes of tests/history.py):
  nrms_naml, nrms_bert, hierec, graph have no get_news_vector: s6 interleaves encode_catalogue (40 and 400 news; nrms_bert: its
      whole table) and the eval forwards instead;
  hierec and graph refuse the pooled loss: no s3p;  nrms_bert has no word table, hence no pad-row flag: no s8;
  hierec's and graph's oracles (oracle/segpool_oracle.py) replay no dropout: the steps held to them run with config.dropout = 0
      (graph: on a freshly encoded catalogue, which the oracle's out-of-batch constants assume); every other step keeps 0.2.

Not bit-reproducible by the project's own documentation, and therefore held to the oracle instead of the twin: the fp16 news
encoder without NRMS_FLAG_PAD_ROW_ZERO (s8b in the fp16 cases of nrms_hip, hierec and graph; nrms_v1's fused fp16 news encoder
needs the flag and reroutes to bf16x3), whose table scatter uses float atomics: that step is held to the family's oracle at the
tolerance of the family's own test, and its forward (scores, loss) is still compared bit for bit.

The project's reproducibility claims are kept: no word id occurs more than 64 times in a call (n_words = 30000;
tests/test_history_host.py asserts the bincount), NRMS_ATOMIC_SCATTER is unset, the padding row is zero except in s8."""
import time

import pytest

from tests import history as hs
from tests.guarded import POISONS

pytestmark = pytest.mark.gpu

CASES = {
    "nrms-d60-fp32": lambda: hs.NrmsFamily("fp32"),
    "nrms-d60-bf16x3": lambda: hs.NrmsFamily("bf16x3"),
    "nrms-d60-fp16": lambda: hs.NrmsFamily("fp16"),
    "nrms-d60-fp16-user16": lambda: hs.NrmsFamily("fp16", fp16_user=True),
    # d = 300: the fp16 pitches have real padding columns, 300 to 319
    "nrms-d300-bf16x3": lambda: hs.NrmsFamily("bf16x3", d=300, heads=10, q=200),
    "nrms-d300-fp16": lambda: hs.NrmsFamily("fp16", d=300, heads=10, q=200),
    "v1-bf16x3": lambda: hs.V1Family("bf16x3"),
    "v1-fp16-news16": lambda: hs.V1Family("fp16"),
    "naml-fp32": lambda: hs.NamlFamily("fp32"),
    "naml-bf16x3": lambda: hs.NamlFamily("bf16x3"),
    "bert-bf16x3": lambda: hs.BertFamily("bf16x3"),
    "hierec-bf16x3": lambda: hs.HieRecFamily("bf16x3"),
    "hierec-fp16": lambda: hs.HieRecFamily("fp16"),
    "graph-bf16x3": lambda: hs.GraphFamily("bf16x3"),
    "graph-fp16": lambda: hs.GraphFamily("fp16"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_results_do_not_depend_on_earlier_calls(case, monkeypatch):
    monkeypatch.delenv("NRMS_ATOMIC_SCATTER", raising=False)
    fam = CASES[case]()
    t0 = time.time()
    for poison in POISONS:
        hs.run_script(fam, poison)
    print("history %s: %.1f s for %d poisons" % (case, time.time() - t0, len(POISONS)))
