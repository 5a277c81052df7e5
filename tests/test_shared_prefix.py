"""Shared-prefix decode attention without a GPU: ``reference.shared_prefix_plan`` (the
definition the plan kernel is held to, and the CPU path) on hand-written block tables, and an
engine with the switch on against one without it."""
import pytest
import torch

from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.ops import reference as R

BS = 16
# name -> (block_tables, context_lens, (header, members, lo))
PLAN_CASES = {
    "all_share_3": ([[7, 3, 9, 11], [7, 3, 9, 12], [7, 3, 9, 13], [7, 3, 9, 0]],
                    [60, 52, 64, 49], ([48, 4], [0, 1, 2, 3], [48, 48, 48, 48])),
    "majority_and_two_outliers": ([[5, 6, 0], [2, 4, 8], [2, 4, 9], [1, 4, 0], [2, 4, 10]],
                                  [20, 40, 45, 30, 33],
                                  ([32, 3], [1, 2, 4, -1, -1], [0, 32, 32, 0, 32])),
    "all_distinct": ([[1, 2], [3, 4], [5, 6]], [20, 20, 20], ([0, 1], [0, -1, -1], [0, 0, 0])),
    "one_row": ([[4, 5, 6]], [40], ([0, 1], [0], [0])),
    # three equal columns, but row 0's newest token is the first of the third block
    "context_ends_one_past_the_run": ([[3, 8, 9], [3, 8, 9], [3, 8, 9]], [33, 48, 48],
                                      ([32, 3], [0, 1, 2], [32, 32, 32])),
    # block 0 is a real block; the zero padding after row 2's two blocks ends nothing early
    "block_0_shared_zero_padding": ([[0, 2, 4, 0, 0], [0, 2, 5, 0, 0], [0, 2, 0, 0, 0]],
                                    [40, 45, 33], ([32, 3], [0, 1, 2], [32, 32, 32])),
    # the rows that pad a captured batch (context 0, a table of zeros) outnumber a group that
    # starts at block 0: they neither lead nor join it, nor bound its run
    "padding_rows_behind_block_0": ([[0, 2, 4], [0, 2, 5], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                                    [40, 45, 0, 0, 0],
                                    ([32, 2], [0, 1, -1, -1, -1], [32, 32, 0, 0, 0])),
    "padding_rows_alone": ([[0, 0], [0, 0]], [0, 0], ([0, 0], [-1, -1], [0, 0])),
}


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_reference_plan(name):
    tables, ctx, want = PLAN_CASES[name]
    got = R.shared_prefix_plan(torch.tensor(tables, dtype=torch.int32),
                               torch.tensor(ctx, dtype=torch.int32), BS)
    assert [g.tolist() for g in got] == [list(w) for w in want]
    assert all(g.dtype == torch.int32 for g in got)


def test_engine_tokens_unchanged_on_cpu():
    sys_prompt = list(range(300, 345))                       # 2 full blocks + 13 tokens
    tails = [[1, 2, 3], [4, 5, 6, 7, 8, 9], list(range(40, 60))]
    sp = SamplingParams(max_length=70, do_sample=False, ignore_eos=True)
    toks = []
    for on in (None, True):
        eng = LLMEngine("llama-tiny128", device="cpu", dtype=torch.float32, max_batch=8,
                        max_model_len=128, num_blocks=64, num_layers=2, shared_prefix=on)
        eng.scheduler.prefix_caching = True
        assert eng.stats()["shared_prefix"] is bool(on)
        eng.generate([sys_prompt + [7]], sp)
        toks.append([o.all_ids for o in eng.generate([sys_prompt + t for t in tails], sp)])
        assert (eng.model.last_shared_plan is not None) is bool(on)
    assert toks[0] == toks[1]
