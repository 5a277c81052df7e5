"""Qwen3-MoE on the GPU: the wave-per-token route with up to 256 experts and optional
renormalisation, the grouped GEMMs on the compact tile-list grid against the dense grid (bit
for bit), an expert-parallel shard of 128 experts, the fused combine + add + RMSNorm at hidden
2048, and the model and the engine against HF transformers' ``Qwen3MoeForCausalLM`` in fp32."""
import itertools

import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import get_config
from distributed_llm_inferencing_amd.models.weights import from_hf_state_dict
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

from hf_helpers import our_last_logits
from test_qwen3_moe import hf_config, hf_qwen3_moe

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PROMPT60 = [(7 * i + 3) % 1024 for i in range(60)]
PROMPT14 = PROMPT60[:14]


def rnd(*shape, dev, scale=1.0, dtype=BF):
    return (torch.randn(*shape, device=dev) * scale).to(dtype)


def close(a, b, rtol=2e-2, atol=2e-2):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    assert err <= tol, f"max err {err} > tol {tol}"


# ------------------------------------------------------------------------------ route
def _tie_free_logits(T, E, dev, seed):
    """Each row a random permutation of the E values (i - E/2) / 16: exact in bf16 for
    E <= 256, neighbours 6 % apart in probability, so the reference alone decides every pick."""
    g = torch.Generator().manual_seed(seed)
    vals = (torch.arange(E, dtype=torch.float32) - E / 2) / 16
    rows = torch.stack([vals[torch.randperm(E, generator=g)] for _ in range(T)])
    assert torch.equal(rows.to(BF).float(), rows)
    return rows.to(BF).to(dev)


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("T,E,k", [(1, 128, 8), (37, 128, 8), (130, 96, 8), (5, 256, 8),
                                   (64, 65, 3)])
def test_moe_route_many_experts(gpu, T, E, k, norm):
    """Up to 4 experts per lane (e = lane + 64 i), with and without the renormalisation."""
    rl = torch.cat([_tie_free_logits(T, E, gpu, 100 * E + T),
                    torch.zeros(1, E, dtype=BF, device=gpu)])         # + one all-tie row
    w, ids = ops.moe_route(rl, k, norm)
    rw, rids = R.router_topk(rl, k, norm)
    assert torch.equal(ids[:T].long().sort(-1).values, rids[:T].long().sort(-1).values)
    close(w.sort(-1).values, rw.sort(-1).values, rtol=1e-3, atol=1e-3)
    assert ids[T].tolist() == list(range(k))              # lowest index on ties
    # the weight of pick j is the softmax value of expert ids[j] (renormalised or not)
    p = rl.float().softmax(-1).gather(1, ids.long())
    close(w, p / p.sum(-1, keepdim=True) if norm else p, rtol=1e-3, atol=1e-3)
    if norm:
        assert torch.allclose(w.sum(-1), torch.ones(T + 1, device=gpu), atol=1e-5)
    else:
        assert bool((w.sum(-1) < 1).all())


@pytest.mark.parametrize("T,E,k", [(129, 8, 2), (5, 64, 2), (64, 64, 8)])
def test_moe_route_default_is_unchanged(gpu, T, E, k):
    """E <= 64 with the renormalisation: against the reference as the existing route tests, and
    the call that passes the new argument gives the bits of the call that does not."""
    torch.manual_seed(9)
    rl = rnd(T, E, dev=gpu)
    rl[0] = 0
    w0, i0 = ops.moe_route(rl, k)
    w1, i1 = ops.moe_route(rl, k, True)
    assert torch.equal(w0, w1) and torch.equal(i0, i1)
    rw, rids = R.router_topk(rl, k)
    assert torch.equal(i0[1:].long().sort(-1).values, rids[1:].long().sort(-1).values)
    assert i0[0].tolist() == list(range(k))
    close(w0.sort(-1).values, rw.sort(-1).values, rtol=1e-3, atol=1e-3)
    assert torch.allclose(w0.sum(-1), torch.ones(T, device=gpu), atol=1e-5)
    wn, inn = ops.moe_route(rl, k, False)                 # same picks, weights not renormalised
    assert torch.equal(inn, i0)
    close(wn / wn.sum(-1, keepdim=True), w0, rtol=1e-5, atol=1e-6)


def test_moe_route_limits(gpu):
    rl = torch.zeros(2, 257, dtype=BF, device=gpu)
    with pytest.raises(RuntimeError, match="dli_moe_route"):
        ops.moe_route(rl, 8)                              # E > 256
    with pytest.raises(RuntimeError, match="dli_moe_route"):
        ops.moe_route(rl[:, :128].contiguous(), 9)        # k > 8 past 64 experts


# ------------------------------------------------------------------------------ tile list
D_, F_, E_ = 256, 64, 128
SENT = 777.0
LIST_TILES_TESTED = sorted(t for t in G.GATHER_TILES if G.TILES[t][0] <= 128)


def _routings(bm):
    """Per-expert row counts: most experts empty and the edge sizes of a bm-row tile; every
    expert non-empty, which fills the list as far as it goes (E non-empty experts of
    q_e bm + r_e rows, r_e >= 1, make E + sum q_e items while ceil(n / bm) >= sum q_e + 1, so
    the bound ceil(n / bm) + E is never reached exactly: here 129 items of at most 131 / 132);
    a single non-empty expert."""
    edge = [0] * E_
    for e, c in ((3, 1), (17, bm - 1), (64, bm), (90, bm + 1), (127, 2 * bm + 3)):
        edge[e] = c
    full = [1] * E_
    full[5] = bm + 1
    one = [0] * E_
    one[77] = bm + 5
    return {"edge": edge, "full": full, "one": one}


@pytest.fixture(scope="module")
def list_case(gpu):
    """Weights, and per (bm, routing): the expert of each row (5 padding rows with id -1 are
    dropped, so the buffers have rows past the routed total), what the align kernel wrote for
    it (offsets, positions, rows, tile list) and the reference output."""
    torch.manual_seed(61)
    wgu = rnd(E_, 2 * F_, D_, dev=gpu, scale=0.05)
    wd = rnd(E_, D_, F_, dev=gpu, scale=0.05)
    cases = {}
    for bm in (64, 128):
        for name, counts in _routings(bm).items():
            g = torch.Generator().manual_seed(bm + len(name))
            ids = torch.tensor([e for e, c in enumerate(counts) for _ in range(c)] + [-1] * 5,
                               dtype=torch.int32)
            ids = ids[torch.randperm(ids.numel(), generator=g)].to(gpu)
            n = ids.numel()
            x = rnd(n, D_, dev=gpu)
            off = torch.empty(E_ + 1, dtype=torch.int32, device=gpu)
            pos = torch.empty(n, dtype=torch.int32, device=gpu)
            src = torch.full((n,), -7, dtype=torch.int32, device=gpu)
            cap = G.max_items(n, E_, bm)
            tl = torch.full((1 + cap, 2), -9, dtype=torch.int32, device=gpu)
            ops._native_call("dli_moe_align_tiles", ops._p(off), ops._p(pos), ops._p(src),
                             ops._p(ids), n, 1, 0, E_, ops._p(tl), bm, cap, None, 0, 0,
                             ops._st())
            ones = torch.ones(n, 1, dtype=torch.float32, device=gpu)
            ref = R.moe_mlp(x, wgu, wd, ones, ids.view(n, 1))
            cases[bm, name] = dict(counts=counts, ids=ids, n=n, x=x, off=off, pos=pos, src=src,
                                   tl=(tl, cap), ref=ref)
    return wgu, wd, cases


@pytest.mark.parametrize("bm", [64, 128])
def test_align_writes_the_tile_list(gpu, list_case, bm):
    """offsets / positions as the plain align, and the list the host builds from the counts:
    one (expert, first row) per bm rows of every non-empty expert, experts ascending."""
    _, _, cases = list_case
    for name in ("edge", "full", "one"):
        c = cases[bm, name]
        counts, n = c["counts"], c["n"]
        off2, pos2 = torch.empty_like(c["off"]), torch.empty_like(c["pos"])
        src2 = torch.empty_like(c["src"])
        ops._native_call("dli_moe_align", ops._p(off2), ops._p(pos2), ops._p(src2),
                         ops._p(c["ids"]), n, 1, 0, E_, ops._st())
        assert torch.equal(c["off"], off2)
        assert c["off"].tolist() == [0] + list(itertools.accumulate(counts))
        total = sum(counts)
        pos = c["pos"].long()
        assert bool(((pos >= 0) == (c["ids"] >= 0)).all())
        kept = pos[pos >= 0]
        assert sorted(kept.tolist()) == list(range(total))
        assert torch.equal(c["src"][kept].long(), (pos >= 0).nonzero().flatten())
        want, _ = G.host_tile_list(counts, bm, gpu)
        tl, cap = c["tl"]                                 # sized for n, the padding rows included
        items = int(want[0, 0])
        assert items == sum(-(-x // bm) for x in counts) < cap
        assert torch.equal(tl[:1 + items], want[:1 + items])
        assert bool((tl[1 + items:] == -9).all())         # nothing written past the count
        if name == "full":
            assert items == E_ + 1 >= cap - 3


@pytest.mark.parametrize("tile", LIST_TILES_TESTED)
def test_tile_list_grid_equals_dense_grid(gpu, list_case, tile):
    """Every <= 128-row tile of the generic family: the gather form (SiLU gate/up through the
    row permutation), the plain grouped call (down) and the 2-split fp16 slab store on the
    compact grid give the bytes of the dense grid, rows past the routed total keep their
    sentinel, and the chain is close to the reference MoE layer."""
    wgu, wd, cases = list_case
    bm = G.TILES[tile][0]
    plan1, plan2 = G.GemmPlan("dli", tile, 1), G.GemmPlan("dli", tile, 2)
    silu = G.tile_ok(tile, "silu_mul")
    for name in ("edge", "full", "one"):
        c = cases[bm, name]
        n, x, off, src, tl = c["n"], c["x"], c["off"], c["src"], c["tl"]
        total = sum(c["counts"])
        # ---- gather form
        act = {}
        if silu:
            for form in ("dense", "list"):
                a = torch.full((n, F_), SENT, dtype=BF, device=gpu)
                if form == "dense":
                    ops._native_call("dli_gemm_grouped_gather", ops._p(x), x.stride(0),
                                     ops._p(wgu), wgu.stride(-2), ops._p(a), a.stride(0), n,
                                     2 * F_, D_, tile, ops._p(src), ops._p(off), E_, ops._st())
                else:
                    ops._native_call("dli_gemm_grouped_list", ops._p(x), x.stride(0),
                                     ops._p(wgu), wgu.stride(-2), ops._p(a), a.stride(0), n,
                                     2 * F_, D_, G.EPI["silu_mul"], tile, 1, ops._p(src), None,
                                     ops._p(off), E_, ops._p(tl[0]), tl[1], ops._st())
                act[form] = a
            assert torch.equal(act["dense"], act["list"]), (name, "gather")
            assert bool((act["list"][total:] == SENT).all()), name
            a_in = act["list"]
        else:                             # a tile without the SiLU pairing: its down GEMM only
            xp = torch.zeros(n, D_, dtype=BF, device=gpu)
            xp[:total] = x[src[:total].long()]
            a_in = R.silu_mul(torch.cat([R.linear(xp[off[e]:off[e + 1]], wgu[e])
                                         for e in range(E_)] + [xp.new_zeros(n - total, 2 * F_)]))
        # ---- plain grouped call (the down projection)
        y = {}
        for form in ("dense", "list"):
            o = torch.full((n, D_), SENT, dtype=BF, device=gpu)
            ops._gemm_native(a_in, wd, "none", out=o, plan=plan1, groups=E_, group_off=off,
                             rows_per_group=n, tile_list=tl if form == "list" else None)
            y[form] = o
        assert torch.equal(y["dense"], y["list"]), (name, "plain")
        assert bool((y["list"][total:] == SENT).all()), name
        pos = c["pos"].long()
        out = torch.zeros(n, D_, dtype=BF, device=gpu)
        out[pos >= 0] = y["list"][pos[pos >= 0]]
        close(out, c["ref"], rtol=3e-2, atol=3e-2)
        # ---- 2-split fp16 slabs (K = 256: x against the gate/up weight as a plain matrix)
        xp = torch.zeros(n, D_, dtype=BF, device=gpu)
        xp[:total] = x[src[:total].long()]
        ws = {}
        for form in ("dense", "list"):
            s = torch.full((2, n, 2 * F_), 0x7b55, dtype=torch.int16, device=gpu)
            if form == "dense":
                ops._native_call("dli_gemm", ops._p(xp), xp.stride(0), ops._p(wgu),
                                 wgu.stride(-2), None, 2 * F_, n, 2 * F_, D_, G.EPI["slab16"],
                                 tile, 2, None, ops._p(s), ops._p(off), E_, ops._st())
            else:
                ops._native_call("dli_gemm_grouped_list", ops._p(xp), xp.stride(0), ops._p(wgu),
                                 wgu.stride(-2), None, 2 * F_, n, 2 * F_, D_, G.EPI["slab16"],
                                 tile, 2, None, ops._p(s), ops._p(off), E_, ops._p(tl[0]), tl[1],
                                 ops._st())
            ws[form] = s
        assert torch.equal(ws["dense"], ws["list"]), (name, "slabs")
        assert bool((ws["list"][:, total:] == 0x7b55).all()), name
        unsplit = ops._gemm_native(xp, wgu, "none", plan=plan1, groups=E_, group_off=off,
                                   rows_per_group=n, tile_list=tl)
        summed = ws["list"].view(torch.float16).float().sum(0) * 16
        close(summed[:total], unsplit[:total], rtol=3e-2, atol=3e-2)
        # ---- split with an output: slabs + the reduce kernel, as the dense call
        r2 = [ops._gemm_native(xp, wgu, "none", plan=plan2, groups=E_, group_off=off,
                               rows_per_group=n, tile_list=t)[:total] for t in (None, tl)]
        assert torch.equal(r2[0], r2[1]), (name, "split + reduce")


def test_list_form_is_refused_where_it_does_not_apply(gpu, list_case):
    wgu, wd, cases = list_case
    c = cases[64, "one"]
    a = torch.zeros(c["n"], F_, dtype=BF, device=gpu)
    tl, cap = c["tl"]
    with pytest.raises(RuntimeError, match="dli_gemm_grouped_list"):       # bound too small
        ops._gemm_native(a, wd, "none", plan=G.GemmPlan("dli", 1, 1), groups=E_,
                         group_off=c["off"], rows_per_group=c["n"], tile_list=(tl, E_))
    with pytest.raises(RuntimeError, match="dli_gemm_grouped_list"):       # 8-phase family
        ops._gemm_native(a, wd, "none", plan=G.GemmPlan("dli", 28, 1), groups=E_,
                         group_off=c["off"], rows_per_group=c["n"], tile_list=(tl, cap))
    assert G.list_plan(G.GemmPlan("dli", 1, 1), 128) and G.list_plan(G.GemmPlan("dli", 1, 1), 9)
    assert not G.list_plan(G.GemmPlan("dli", 1, 1), 8)                     # Mixtral: dense grid
    assert not G.list_plan(G.GemmPlan("dli", 28, 1), 128)


# ------------------------------------------------------------------------------ moe_mlp
@pytest.mark.parametrize("T", [1, 37, 300])
def test_moe_mlp_128_experts(gpu, T):
    """The whole layer through the list form (default plans: 64-row tiles up to ~50 rows per
    expert, T = 300 with 8 picks takes more than one item on the busiest experts)."""
    torch.manual_seed(67 + T)
    E, k, D, F = 128, 8, 256, 64
    x = rnd(T, D, dev=gpu)
    rw, rids = R.router_topk(rnd(T, E, dev=gpu, scale=2.0), k)
    wgu = rnd(E, 2 * F, D, dev=gpu, scale=0.05)
    wd = rnd(E, D, F, dev=gpu, scale=0.05)
    assert G.list_plan(G.grouped_plan(T * k, 2 * F, D, "silu_mul", E), E)
    close(ops.moe_mlp(x, wgu, wd, rw, rids), R.moe_mlp(x, wgu, wd, rw, rids),
          rtol=3e-2, atol=3e-2)


def test_moe_mlp_two_tile_heights(gpu):
    """Gate/up and down on tiles of different heights: the align writes both lists."""
    torch.manual_seed(71)
    T, E, k, D, F = 64, 128, 8, 256, 64
    x = rnd(T, D, dev=gpu)
    rw, rids = R.router_topk(rnd(T, E, dev=gpu, scale=2.0), k)
    wgu = rnd(E, 2 * F, D, dev=gpu, scale=0.05)
    wd = rnd(E, D, F, dev=gpu, scale=0.05)
    keys = {(G._bucket(T * k), 2 * F, D, "silu_mul", E): G.GemmPlan("dli", 1, 1),
            (G._bucket(T * k), D, F, "none", E): G.GemmPlan("dli", 2, 1)}
    old = {key: G._grouped_cache.get(key) for key in keys}
    G._grouped_cache.update(keys)
    try:
        out = ops.moe_mlp(x, wgu, wd, rw, rids)
    finally:
        for key, p in old.items():
            if p is None:
                G._grouped_cache.pop(key, None)
            else:
                G._grouped_cache[key] = p
    close(out, R.moe_mlp(x, wgu, wd, rw, rids), rtol=3e-2, atol=3e-2)


def test_moe_mlp_expert_parallel_shard(gpu):
    """Experts 32..47 of 128 on this rank: picks elsewhere contribute nothing."""
    torch.manual_seed(73)
    T, E, k, D, F, e0, el = 37, 128, 8, 256, 64, 32, 16
    x = rnd(T, D, dev=gpu)
    rw, rids = R.router_topk(rnd(T, E, dev=gpu, scale=2.0), k)
    wgu = rnd(el, 2 * F, D, dev=gpu, scale=0.05)
    wd = rnd(el, D, F, dev=gpu, scale=0.05)
    local = (rids >= e0) & (rids < e0 + el)
    assert bool(local.any()) and not bool(local.any(-1).all())      # some tokens have none
    out = ops.moe_mlp(x, wgu, wd, rw, rids, expert_offset=e0)
    close(out, R.moe_mlp(x, wgu, wd, rw, rids, e0), rtol=3e-2, atol=3e-2)
    assert bool((out[~local.any(-1)] == 0).all())


def test_autotune_grouped_128_groups(gpu):
    """The tuner at 128 groups: short tiles only, timed on the list form; its pick runs."""
    torch.manual_seed(79)
    E, N, K, rows = 128, 128, 256, 296
    w = rnd(E, N, K, dev=gpu, scale=0.05)
    key = (G._bucket(rows), N, K, "silu_mul", E)
    assert key not in G._grouped_cache
    try:
        best = G.autotune_grouped(rows, w, "silu_mul", iters=2)
        assert best is not None and G.grouped_plan(rows, N, K, "silu_mul", E) == best[0]
        assert G.TILES[best[0].tile][0] <= 2 * max(64, rows // E + 32)
    finally:
        G._grouped_cache.pop(key, None)


# ------------------------------------------------------------------------------ fused combine
@pytest.mark.parametrize("splits", [2, 4])
def test_moe_combine_fused_with_next_norm_dim_2048(gpu, splits):
    """The deferred combine inside the next layer's add + RMSNorm at hidden 2048 (256 threads x
    8 columns) == the plain combine, then the add + RMSNorm kernel. No split plan is eligible
    at Qwen3-MoE's down projection (K = 768), so the plan is forced."""
    torch.manual_seed(47)
    T, E, k, D, F = 96, 16, 2, 2048, 512
    x = rnd(T, D, dev=gpu)
    logits = rnd(T, E, dev=gpu)
    logits[:, 5] = -30.0                          # expert 5 is never picked
    rw, rids = R.router_topk(logits, k)
    wgu = rnd(E, 2 * F, D, dev=gpu, scale=0.05)
    wd = rnd(E, D, F, dev=gpu, scale=0.05)
    key = (G._bucket(T * k), D, F, "none", E)
    old = G._grouped_cache.get(key)
    G._grouped_cache[key] = G.GemmPlan("dli", 12, splits)
    calls = []
    real = ops._native_call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    ops._native_call = spy
    try:
        pend = ops.moe_mlp(x, wgu, wd, rw, rids, defer_combine=True)
        assert isinstance(pend, ops.MoEPending)
        r0, nw = rnd(T, D, dev=gpu), (1.0 + 0.1 * rnd(D, dev=gpu)).to(BF)
        r1, r2, r3 = r0.clone(), r0.clone(), r0.clone()
        plain = pend.materialize()
        close(plain, R.moe_mlp(x, wgu, wd, rw, rids), rtol=3e-2, atol=3e-2)
        out_b = ops.add_rmsnorm(plain, r2, nw, 1e-5)
        out_a = ops.add_rmsnorm(pend, r1, nw, 1e-5)
        assert torch.equal(r1, r2)
        close(out_a, out_b, rtol=1e-2, atol=1e-2)
        assert pend.add_rmsnorm(r3, None, 1e-5) is None
        assert torch.equal(r3, r2)
        assert calls.count("dli_moe_combine_add_rmsnorm") == 2       # not the fallback
    finally:
        ops._native_call = real
        if old is None:
            G._grouped_cache.pop(key, None)
        else:
            G._grouped_cache[key] = old


# ------------------------------------------------------------------------------ model, engine
@pytest.mark.parametrize("name", ["qwen3-moe-tiny", "qwen3-moe-tiny128"])
def test_gpu_logits_close_to_hf_fp32(gpu, name):
    cfg = get_config(name)
    hm = hf_qwen3_moe(cfg)
    with torch.no_grad():
        ref = hm(torch.tensor([PROMPT14])).logits[0, -1]
    params = from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.bfloat16)
    params = {k: v.to(gpu) for k, v in params.items()}
    ours = our_last_logits(cfg, params, PROMPT14, device=gpu).cpu()
    err = (ours - ref).abs().max().item()
    assert err < 0.05 * ref.abs().max().item() + 0.02, err
    assert ours.argmax() == ref.argmax() or (ref.topk(2).values.diff().abs() < 0.05).item()


def test_graph_decode_equals_eager(gpu, monkeypatch):
    """The list-form launches under capture: their grid depends on shapes only."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")          # same GEMM plans on both sides
    ids = [5, 17, 99, 3, 250, 7, 8, 1000, 42, 11, 600, 3, 3, 9]
    prompts = [ids[:5], ids[:9], ids[3:14], ids[:2]]
    sp = SamplingParams(max_length=40, temperature=0.8, top_k=50, top_p=0.95, seed=123,
                        ignore_eos=True)
    outs = []
    for graphs in (False, True):
        eng = LLMEngine("qwen3-moe-tiny", device="cuda", max_batch=8, max_model_len=128,
                        num_blocks=64, use_graphs=graphs, seed=3)
        outs.append([o.output_ids for o in eng.generate(prompts, sp)])
        assert bool(eng.runner.graphs) == graphs, "no decode graph was captured"
    assert outs[0] == outs[1]


# (model seed, prompt offsets into PROMPT60) chosen on the CPU in fp32 among seeds 0-39 and the
# offsets 0, 3, .. 42 of qwen3-moe-tiny128 (the twin with tied embeddings, whose continuations
# are decisive): along each 16-token prompt's greedy continuation of 24 tokens the top-two
# logits of the HF twin are never closer than 0.252 / 0.237 / 0.182 / 0.179, 6-10 times the
# near-tie bound below (at most 0.029), and the bf16 CPU engine reproduces all four.
# The routing cannot be given such a margin: over the 624 (token, layer) routings of these
# continuations the 4th and 5th router logits of the fp32 twin come as close as 0.0002 (1.6e-5
# in probability) while the bf16 CPU path's router logits differ from fp32 by up to 0.0103, and
# 13 of the 624 pick sets differ there — with tens of experts some token always has two
# candidates for the last pick within rounding. Such a swap exchanges two experts of nearly
# equal, small weight; it is the logit margin above that keeps the tokens.
GREEDY_SEED, GREEDY_OFFSETS = 20, (18, 36, 12, 33)


def test_engine_greedy_tokens_match_hf_fp32(gpu):
    """4 prompts x 24 new tokens through the bf16 engine on the GPU against HF fp32
    ``generate`` (qwen3-moe-tiny128: 16 experts, top-4, weights not renormalised). Two requests decode (graph replays)
    before the other two arrive. A prompt may differ only from a step where the reference's
    top-two logits are a near tie, and at most one may differ."""
    cfg = get_config("qwen3-moe-tiny128")
    hm = hf_qwen3_moe(cfg, seed=GREEDY_SEED)
    params = from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.bfloat16)
    eng = LLMEngine(cfg, device="cuda", params=params, max_batch=4, max_model_len=128,
                    num_blocks=32)
    assert eng.runner.use_graphs
    prompts = [PROMPT60[o:o + 16] for o in GREEDY_OFFSETS]
    sp = SamplingParams(max_new_tokens=24, do_sample=False, ignore_eos=True)
    rids = [eng.add_request(p, sp) for p in prompts[:2]]
    done = {}
    for _ in range(4):
        done.update({o.request_id: o for o in eng.step()})
    rids += [eng.add_request(p, sp) for p in prompts[2:]]
    while eng.has_work():
        done.update({o.request_id: o for o in eng.step()})
    assert eng.stats.decode_steps >= 20, eng.stats
    assert eng.runner.graphs, "no decode graph was captured"
    differ = 0
    for p, rid in zip(prompts, rids):
        got = list(p) + list(done[rid].output_ids)
        with torch.no_grad():
            ref = hm.generate(torch.tensor([p]), max_length=40, do_sample=False,
                              eos_token_id=None, pad_token_id=0)[0].tolist()
        assert len(got) == len(ref) == 40
        if got == ref:
            continue
        differ += 1
        n = next(i for i, (a, b) in enumerate(zip(got, ref)) if a != b)
        with torch.no_grad():
            top = hm(torch.tensor([ref[:n]])).logits[0, -1].topk(2).values
        assert (top[0] - top[1]).item() < 0.01 * top[0].abs().item() + 0.01, (n, top)
    assert differ <= 1, differ


def test_real_shape_layers_close_to_hf_fp32(gpu):
    """Qwen3-30B-A3B at its real layer shapes (hidden 2048, 32 heads / GQA 4 / head 128, 128
    experts x 768, top-8) and vocabulary, 2 layers: prefill logits of the HIP path against HF
    transformers in fp32 on the same weights."""
    import transformers as tf
    torch.manual_seed(0)
    cfg = get_config("qwen3-30b-a3b", num_layers=2)
    with torch.device(gpu):
        hm = tf.Qwen3MoeForCausalLM(hf_config(cfg)).float().eval()
    ids = PROMPT14 + [1234, 4321, 777]
    with torch.no_grad():
        ref = hm(torch.tensor([ids], device=gpu)).logits[0, -1].float().cpu()
        params = from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.bfloat16)
    del hm
    params = {k: v.to(gpu) for k, v in params.items()}
    ours = our_last_logits(cfg, params, ids, device=gpu).float().cpu()
    err = (ours - ref).abs().max().item()
    assert err < 0.05 * ref.abs().max().item() + 0.02, err
