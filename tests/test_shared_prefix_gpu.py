"""Shared-prefix decode attention on the GPU (attention_decode_shared.hip): the plan kernel
against ``reference.shared_prefix_plan`` integer for integer, and ``ops.decode_attention(...,
shared=plan)`` against ``reference.decode_attention`` on float64 copies, eager, under graph
replay with rewritten block tables, with a count witness across the seam, and in the model."""
import math

import pytest
import torch

import attention_witness as AW
from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.batch import DECODE, DeviceBatch
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models.configs import get_config
from distributed_llm_inferencing_amd.models.model import TransformerLM
from distributed_llm_inferencing_amd.ops import reference as R
from test_shared_prefix import PLAN_CASES

pytestmark = pytest.mark.gpu
BS, HD, NBLK = 16, 128, 512


def close(a, b, rtol=2e-2, atol=2e-2):          # test_decode_attention_paged's tolerance
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    assert err <= tol, f"max err {err} > tol {tol}"


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_plan_equals_the_reference(gpu, name):
    tables, ctx, _ = PLAN_CASES[name]
    bt = torch.tensor(tables, dtype=torch.int32, device=gpu)
    cl = torch.tensor(ctx, dtype=torch.int32, device=gpu)
    got, want = ops.shared_prefix_plan(bt, cl, BS), R.shared_prefix_plan(bt.cpu(), cl.cpu(), BS)
    for g, w in zip(got, want):
        assert g.dtype == torch.int32 and torch.equal(g.cpu(), w)


def batch_tables(members, shared, width, seed, others=2, nblk=NBLK):
    """(tables [members + others, width], ctx): ``members`` rows start with the same ``shared``
    blocks (block 0 the first of them) and go on with private blocks for a suffix of 1..50
    tokens, row 0's being the new token alone; ``others`` rows share nothing. Zero padding."""
    g = torch.Generator().manual_seed(seed)
    ids = (1 + torch.randperm(nblk - 1, generator=g)).tolist()
    run = ([0] + [ids.pop() for _ in range(shared - 1)]) if shared else []
    rows, ctx = [], []
    for r in range(members + others):
        suffix = 1 if r == 0 else 1 + int(torch.randint(0, 50, (1,), generator=g))
        head = run if r < members else [ids.pop() for _ in range(shared)]
        n = shared * BS + suffix
        row = head + [ids.pop() for _ in range(-(-n // BS) - shared)]
        rows.append(row + [0] * (width - len(row)))
        ctx.append(n)
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(ctx, dtype=torch.int32)


@pytest.fixture(scope="module")
def pool(gpu):
    """One random cache pool and query rows per head shape; any table over it is a sequence."""
    g = torch.Generator(device=gpu).manual_seed(3)
    made = {}

    def get(hq, hkv):
        if (hq, hkv) not in made:
            kv = torch.randn(2, NBLK, hkv, BS, HD, device=gpu, generator=g).to(torch.bfloat16)
            qkv = torch.randn(72, (hq + 2 * hkv) * HD, device=gpu, generator=g).to(torch.bfloat16)
            made[hq, hkv] = (kv[0], kv[1], qkv)
        return made[hq, hkv]
    return get


def reference(qkv, kc, vc, bt, cl, hq):
    q = qkv[:, :hq * HD].reshape(len(qkv), hq, HD).double()
    return R.decode_attention(q, kc.double(), vc.double(), bt, cl, 1 / math.sqrt(HD)).flatten(1)


@pytest.mark.parametrize("shared", [0, 1, 5, 40])
@pytest.mark.parametrize("members", [3, 17, 70])
@pytest.mark.parametrize("hq,hkv", [(8, 2), (4, 4), (16, 1)])
def test_attention_equals_the_reference(gpu, pool, hq, hkv, members, shared):
    kc, vc, qkv = pool(hq, hkv)
    bt, cl = (t.to(gpu) for t in batch_tables(members, shared, 45, 100 * members + shared))
    qkv = qkv[:members + 2]
    plan = ops.shared_prefix_plan(bt, cl, BS)
    assert plan.header.tolist() == [shared * BS, members if shared else 1]
    out = ops.decode_attention(qkv, kc, vc, bt, cl, int(cl.max()), hq, hkv, HD,
                               1 / math.sqrt(HD), shared=plan)
    close(out, reference(qkv, kc, vc, bt, cl, hq))


def test_count_witness_across_the_seam(gpu):
    """q = 0 and V[t, d] = [t mod hd == d]: every key of [0, ctx) counts once, those of the
    last (half) shared tile, tokens 64..79, and of the first suffix tile, from token 80, among
    them; a key dropped or doubled at the seam moves an output element by 1 / ctx."""
    hq, hkv = 8, 2
    sc = AW.decode_count([81, 100, 113, 97], hq, hkv, HD, BS, 0, seed=5)
    kc, vc, bt, cl = AW.device_cache(sc, gpu)
    bt[:, :5] = bt[0, :5].clone()            # K and V follow the position alone: same content
    plan = ops.shared_prefix_plan(bt, cl, BS)
    assert plan.header.tolist() == [80, 4]
    out = ops.decode_attention(AW.device_qkv(sc, hkv, gpu), kc, vc, bt, cl, 113, hq, hkv, HD,
                               1 / math.sqrt(HD), shared=plan)
    AW.check(out, sc, "decode_attention(shared=plan)")


def test_graph_replay_replans(gpu, pool):
    """The plan launch is inside the capture: replays over block tables rewritten in place to
    shared runs of 9, 5, 0 and 9 blocks each match the reference (no stale plan or partials).
    max_context 320 gives two chunks of 128 tokens: the second holds keys at 9 blocks and
    turns neutral at 5 and 0."""
    hq, hkv, members, width = 8, 2, 17, 20
    kc, vc, qkv = pool(hq, hkv)
    qkv = qkv[:members + 2]
    bt, cl = (t.to(gpu) for t in batch_tables(members, 3, width, 1))
    out = torch.empty(members + 2, hq * HD, dtype=torch.bfloat16, device=gpu)

    def step():
        plan = ops.shared_prefix_plan(bt, cl, BS)
        ops.decode_attention(qkv, kc, vc, bt, cl, width * BS, hq, hkv, HD, 1 / math.sqrt(HD),
                             out=out, shared=plan)
        return plan
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan = step()
    for shared in (9, 5, 0, 9):
        nbt, ncl = batch_tables(members, shared, width, 10 + shared)
        bt.copy_(nbt)
        cl.copy_(ncl)
        graph.replay()
        assert int(plan.header[0]) == shared * BS
        close(out, reference(qkv, kc, vc, bt, cl, hq))


def test_model_decode_step(gpu):
    """One llama-tiny128 decode step over 6 sequences that share 3 blocks: the logits with the
    switch on agree with the fused path's, and the step's plan found the 48 shared tokens."""
    cfg = get_config("llama-tiny128", 2)
    lm = TransformerLM.random(cfg, device=gpu, seed=2)
    g = torch.Generator(device=gpu).manual_seed(4)
    kvs = [tuple(torch.randn(2, 64, cfg.num_kv_heads, BS, HD, device=gpu, generator=g)
                 .to(torch.bfloat16).unbind(0)) for _ in range(cfg.num_layers)]
    bt, cl = (t.to(gpu) for t in batch_tables(6, 3, 8, 6, others=0, nblk=64))
    slots = (bt.gather(1, ((cl - 1) // BS).long()[:, None])[:, 0] * BS + (cl - 1) % BS).int()
    b = DeviceBatch(kind=DECODE, num_seqs=6, num_tokens=6,
                    input_ids=torch.arange(5, 11, dtype=torch.int32, device=gpu),
                    positions=cl - 1, slot_mapping=slots, block_tables=bt, context_lens=cl,
                    max_context=int(cl.max()))
    logits = []
    for on in (False, True):
        lm.shared_prefix = on
        logits.append(lm.logits(lm.forward_layers(lm.embed(b), b, kvs), b))
    assert lm.last_shared_plan.header.tolist() == [48, 6]
    close(logits[1], logits[0])


def test_engine_padded_bucket_keeps_the_run(gpu, monkeypatch):
    """Three requests behind a cached 45-token prompt decode in the 4-row graph bucket. Its
    padding row has context 0 and a table of zeros, and block 0 is the prompt's first block:
    the captured plan still finds the 3 members and their 2 shared blocks."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")
    eng = LLMEngine("llama-tiny128", device="cuda", max_batch=8, max_model_len=128,
                    num_blocks=64, num_layers=2, use_graphs=True, lookahead=False,
                    shared_prefix=True)
    eng.scheduler.prefix_caching = True
    prompt = list(range(300, 345))
    sp = SamplingParams(max_new_tokens=6, temperature=0.0, ignore_eos=True)
    eng.generate([prompt + [7]], sp)
    outs = eng.generate([prompt + [t] for t in (1, 2, 3)], sp)
    assert [len(o.output_ids) for o in outs] == [6, 6, 6] and 4 in eng.runner.graphs
    assert eng.model.last_shared_plan.header.tolist() == [32, 3]
    assert eng.model.last_shared_plan.lo.tolist() == [32, 32, 32, 0]
