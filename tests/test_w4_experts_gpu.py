"""The grouped W4 MFMA nibble stream (``dli_gemm_w4_stream_grouped``, tiles 74 / 75) and
``ops.W4Experts`` on the GPU against fp64 / fp32 CPU references from ``reference.unpack_w4``."""
from itertools import accumulate

import pytest
import torch

import test_w4_weights_gpu as dense
from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.models import get_config
from distributed_llm_inferencing_amd.models.weights import quantize_params, random_init, \
    stage_param_shapes
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R
from test_fp8_experts_gpu import clean_plans  # noqa: F401
from test_w4_weights_gpu import BF, close, plan, rnd

pytestmark = pytest.mark.gpu
TILES = sorted(G.W4_STREAM_TILES)
SENT, PAD, TOKENS, N = 777.0, 3, 40, 96      # 96 rows: the last workgroup has clamped groups
AROW = ((7 * torch.arange(200) + 3) % TOKENS).to(torch.int32)


@pytest.fixture
def bf16_calls(monkeypatch):
    """The calls of ``ops.W4Experts.bf16`` (the dequantise pass of a stack) during the test."""
    calls = []
    real = ops.W4Experts.bf16
    monkeypatch.setattr(ops.W4Experts, "bf16", lambda self: (calls.append(1), real(self))[1])
    return calls


def stack(q, s, z, dev="cpu"):
    """(ops.W4Experts on ``dev``, its fp64 value from ``reference.unpack_w4``: (q - z) * s)."""
    E, n, K = q.shape
    qp, sz = R.pack_w4(q.view(E * n, K), s.view(E * n, -1), z.view(E * n, -1))
    uq, us, uz = R.unpack_w4(qp, sz)
    rep = lambda t: t.double().repeat_interleave(128, 1)  # noqa: E731
    return (ops.W4Experts(qp.view(E, n, -1), sz.view(E, n, -1)).to(dev),
            ((uq.double() - rep(uz)) * rep(us)).view(E, n, K))


def random_stack(E, n, K, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return stack(torch.randint(0, 16, (E, n, K), generator=g, dtype=torch.uint8),
                 torch.exp2(torch.rand(E, n, K // 128, generator=g) * 4 - 8).to(torch.float16),
                 torch.randint(0, 16, (E, n, K // 128), generator=g, dtype=torch.uint8), dev)


def product(x, wf, counts, arow):
    off = [0] + list(accumulate(counts))
    src = torch.arange(off[-1]) if arow is None else arow[:off[-1]].long()
    return torch.cat([x.double()[src[off[e]:off[e + 1]]] @ wf[e].t() for e in range(len(counts))])


def run(gpu, x, w, epi, tile, bm, counts, arow=None, tl=None):
    n = sum(counts)
    off = torch.tensor([0] + list(accumulate(counts)), dtype=torch.int32, device=gpu)
    out = torch.full((n + PAD, w.shape[1] // (2 if epi == "silu_mul" else 1)), SENT,
                     dtype=torch.float32 if epi == "f32" else BF, device=gpu)
    ops.grouped_stream(x.to(gpu), w, plan(tile), epi, out, off, n, bm,
                       tl or G.host_tile_list(counts, bm, gpu),
                       None if arow is None else arow.to(gpu))
    return out


def witness(K, bm, permuted):
    """Integers, scales in {1/2, 1, 2}, q / s / z distinct per expert; experts of 0, 1 and
    bm + 1 rows. Every partial sum is below 2^24 in steps of 1/2
    (``test_w4_stream_gpu.test_exact_witness``'s bound), so fp32 equals fp64 or an index is wrong."""
    counts = [0, 1, bm + 1]
    e, n = torch.arange(3)[:, None, None], torch.arange(N)[None, :, None]
    k, grp = torch.arange(K)[None, None, :], torch.arange(K // 128)[None, None, :]
    w, wf = stack(((k + 3 * (k // 8) + 5 * n + 7 * e) % 16).to(torch.uint8),
                  torch.exp2(((n + grp + e) % 3 - 1).float()).to(torch.float16),
                  ((5 * n + 3 * grp + 11 * e) % 16).to(torch.uint8))
    rows = TOKENS if permuted else sum(counts) + PAD
    x = ((torch.arange(rows)[:, None] * 7 + k[0] * 5 + k[0] // 8) % 9 - 4).to(BF)
    arow = AROW if permuted else None
    want = product(x, wf, counts, arow)
    assert torch.equal(want, want.float().double()) and want.abs().max() > 0
    return w, x, arow, counts, want


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("bm", [16, 32, 64])
@pytest.mark.parametrize("tile", TILES)
def test_exact_witness(gpu, tile, bm, permuted):
    for K in (128, 384, 1152):        # one block, fewer than either ring, more than either
        w, x, arow, counts, want = witness(K, bm, permuted)
        y = run(gpu, x, w.to(gpu), "f32", tile, bm, counts, arow)
        assert torch.equal(y[:-PAD].cpu().double(), want), K
        assert bool((y[-PAD:] == SENT).all()), K


@pytest.mark.parametrize("tile", TILES)
def test_untouched_rows(gpu, tile):
    """A one-item list (expert 1's single row) writes that row only: not expert 2's rows inside
    the item's height, the rows past the total or the pairs past the count."""
    w, x, _, counts, want = witness(384, 16, False)
    one, cap = G.host_tile_list(counts, 16, gpu)
    assert one[1:4].tolist() == [[1, 0], [2, 0], [2, 16]]
    one[0, 0] = 1
    y = run(gpu, x, w.to(gpu), "f32", tile, 16, counts, tl=(one, cap))
    assert torch.equal(y[:1].cpu().double(), want[:1]) and bool((y[1:] == SENT).all())


ECOUNTS = [3, 0, 70]
_case = {}


def epi_case(gpu):
    if not _case:
        torch.manual_seed(3)
        (w, wf), x = random_stack(3, N, 768, gpu, 5), rnd(TOKENS, 768, dev=gpu)
        _case[0] = (w, x, product(x.cpu(), wf, ECOUNTS, AROW))
    return _case[0]


@pytest.mark.parametrize("bm", [16, 32, 48, 64])
@pytest.mark.parametrize("epi", ["none", "f32", "silu_mul"])
@pytest.mark.parametrize("tile", TILES)
def test_epilogues(gpu, tile, epi, bm):
    w, x, y = epi_case(gpu)
    out = run(gpu, x, w, epi, tile, bm, ECOUNTS, AROW)
    close(out[:-PAD].cpu(), R.silu_mul(y.to(BF)) if epi == "silu_mul" else y)
    assert bool((out[-PAD:] == SENT).all())


BAD = [dict(tile=70), dict(splits=2), dict(bm=24), dict(max_items=65536), dict(max_items=7),
       dict(N=88), dict(K=704), dict(K=64), dict(ldw=784), dict(ldw=736), dict(lda=772),
       dict(lda=760), dict(sld=5), dict(a=None), dict(a=2), dict(wq=8), dict(sz=2), dict(c=None),
       dict(epi="silu_mul", N=80), dict(epi="bias"), dict(off=None), dict(tl=None)]


@pytest.mark.parametrize("bad", BAD, ids=str)
def test_entry_refuses(gpu, bad):
    w = epi_case(gpu)[0]
    xx = torch.zeros(74, 776, dtype=BF, device=gpu)
    out = torch.full((73, N), SENT, dtype=BF, device=gpu)
    off = torch.tensor([0, 3, 3, 73], dtype=torch.int32, device=gpu)
    tl, cap = G.host_tile_list(ECOUNTS, 16, gpu)
    ptr = lambda t, d=0: None if d is None or t is None else t.data_ptr() + d  # noqa: E731

    def call(tile=74, splits=1, bm=16, max_items=cap, N=N, K=768, ldw=768, lda=776, sld=6, a=0,
             wq=0, sz=0, c=0, epi="none", off=off, tl=tl):
        ops._native_call("dli_gemm_w4_stream_grouped", ptr(xx, a), lda, ptr(w.q_packed, wq),
                         ptr(w.sz, sz), sld, ldw, ptr(out, c), 96, 73, N, K, G.EPI[epi], tile,
                         splits, bm, None, ptr(off), 3, ptr(tl), max_items, ops._st())
    call()
    out.fill_(SENT)
    with pytest.raises(RuntimeError, match="dli_gemm_w4_stream_grouped"):
        call(**bad)
    torch.cuda.synchronize()
    assert cap >= 8 and bool((out == SENT).all())


SHAPES = {"qwen": (16, 4, 256, 128), "mixtral": (4, 2, 256, 256)}     # E, top-k, D, F


@pytest.mark.parametrize("kind,T", [("qwen", 1), ("qwen", 37), ("mixtral", 1), ("mixtral", 37),
                                    ("mixtral", 2048)])      # 4096 rows on 4 experts: prefill
def test_moe_mlp_streams_and_dequantises(gpu, kind, T, bf16_calls, clean_plans):  # noqa: F811
    E, k, D, F = SHAPES[kind]
    (wgu, gf), (wd, df) = random_stack(E, 2 * F, D, gpu, 1), random_stack(E, D, F, gpu, 2)
    torch.manual_seed(T)
    x, n = rnd(T, D, dev=gpu), T * k
    tw, ti = R.router_topk(torch.randn(T, E, device=gpu), k)
    ref = R.moe_mlp(x.float(), gf.float().to(gpu), df.float().to(gpu), tw, ti)

    def pin(p):
        G._grouped_cache[G._grouped_key(n, 2 * F, D, "silu_mul", E, "w4")] = p
        G._grouped_cache[G._grouped_key(n, D, F, "none", E, "w4")] = p
    close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)                  # untuned: tile 74
    if n >= 1024 * E:                                            # prefill-sized: the bf16 image
        assert len(bf16_calls) == 2
        return
    pin(plan(75))
    close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)
    e0, e1 = E // 4, E // 4 + E // 2                             # an expert-range shard
    cut = lambda w: ops.W4Experts(w.q_packed[e0:e1].clone(), w.sz[e0:e1].clone())  # noqa: E731
    close(ops.moe_mlp(x, cut(wgu), cut(wd), tw, ti, e0),
          R.moe_mlp(x.float(), gf[e0:e1].float().to(gpu), df[e0:e1].float().to(gpu), tw, ti, e0))
    assert bf16_calls == []
    wide = torch.zeros(T, 2 * D, dtype=BF, device=gpu)           # a non-contiguous x: gate/up
    wide[:, ::2] = x
    close(ops.moe_mlp(wide[:, ::2], wgu, wd, tw, ti), ref)
    assert len(bf16_calls) == 1
    pin(plan(G.grouped_tile(n, E)))                              # a pinned bf16 plan: both
    close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)
    assert len(bf16_calls) == 3 and all(len(key) == 6 for key in G._grouped_cache)
    pin(plan(70))
    with pytest.raises(ValueError, match="tile 70.*W4Experts"):
        ops.moe_mlp(x, wgu, wd, tw, ti)


def test_model_with_streamed_experts(gpu, clean_plans, monkeypatch):  # noqa: F811
    """``test_w4_weights_gpu``'s engine run on qwen3-moe-tiny128: the GPU logits against the CPU
    engine on the same quantised parameters (it reads their fp32 reconstruction), that test's
    bound and near-tie rule, and graph decode equal to eager."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")
    G.clear_plans()
    cfg = get_config("qwen3-moe-tiny128", 2)
    monkeypatch.setattr(dense, "CFG", cfg)
    shapes = stage_param_shapes(cfg, 0, cfg.num_layers, True, True)
    params = quantize_params(cfg, random_init(shapes, "cpu", BF, seed=11, std=0.05), "w4")
    assert params["layers.0.w_gu"].dim() == 3 and "layers.0.w_down_sz" in params
    prompts = [dense.IDS[i:i + 4 + i] for i in range(8)]
    t_ref, l_ref = dense._run("cpu", params, prompts, monkeypatch, False)
    t_gpu, l_gpu = dense._run("cuda", params, prompts, monkeypatch, False)
    assert dense._run("cuda", params, prompts, monkeypatch, True)[0] == t_gpu
    assert len(l_ref) == len(l_gpu) >= 6
    for i, (a, b) in enumerate(zip(l_gpu, l_ref)):
        err = (a - b).abs().max().item()
        assert err < 0.05 * b.abs().max().item() + 0.02, (i, err)
        if [t[:i + 1] for t in t_gpu] != [t[:i + 1] for t in t_ref]:
            break                      # a near tie flipped a token: later steps see other inputs
    G.clear_plans()


def test_autotune_grouped_pins_under_the_w4_key(gpu, clean_plans):  # noqa: F811
    for (w, _), epi in ((random_stack(4, 512, 256, gpu, 5), "silu_mul"),
                        (random_stack(4, 256, 256, gpu, 6), "none")):
        E, n, K = w.shape
        best = G.autotune_grouped(64, w, epi, iters=2)
        assert G._grouped_cache[G._grouped_key(64, n, K, epi, E, "w4")] == best[0]
        assert G._grouped_key(64, n, K, epi, E) not in G._grouped_cache
