"""Micro-benchmark individual HIP kernels (hot-op iteration harness).

Usage (on a GPU box):  python tools/kbench.py [names...]
Names default to all.  Prints ms/call over 20 timed iterations.
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

import spacy_ray_amd  # noqa: F401  (loads _srx_hip)
from spacy_ray_amd.ops.api import hip_ext

hip = hip_ext()
assert hip is not None
dev = "cuda"
torch.manual_seed(0)


def timeit(name, fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    print(f"{name:32s} {ms:8.3f} ms/call")
    return ms


def bench_mwe():
    T, W = 1000064, 96
    X = torch.randn(T, W, device=dev, dtype=torch.bfloat16)
    Wt = torch.randn(3 * W, 3 * W, device=dev, dtype=torch.bfloat16) * 0.05
    bias = torch.randn(3 * W, device=dev, dtype=torch.bfloat16)
    g = torch.ones(W, device=dev, dtype=torch.bfloat16)
    b = torch.zeros(W, device=dev, dtype=torch.bfloat16)
    starts = torch.zeros(T, device=dev, dtype=torch.uint8)
    ends = torch.zeros(T, device=dev, dtype=torch.uint8)
    starts[::20] = 1
    ends[19::20] = 1
    timeit("mwe_layer_fwd (T=1M,W=96)",
           lambda: hip.mwe_layer_fwd(X, Wt, bias, g, b, starts, ends, None, 1e-5))
    dY = torch.randn(T, W, device=dev, dtype=torch.bfloat16)
    Y, Mout, which, mu, rstd = hip.mwe_layer_fwd(X, Wt, bias, g, b, starts,
                                                 ends, None, 1e-5)
    dm = torch.ones(T, W, device=dev, dtype=torch.bfloat16)
    timeit("mwe_bwd_stage1 (T=1M,W=96)",
           lambda: hip.mwe_bwd_stage1(dY, dm, Mout, g, mu, rstd, which))
    # dX: the composed path (GEMM + seq2col_bwd with the residual) against
    # the fused kernel, on the same dPre
    dPre = hip.mwe_bwd_stage1(dY, dm, Mout, g, mu, rstd, which)[0]
    dX3 = dPre.mm(Wt)
    timeit("dPre.mm(weight) (T=1M,W=96)", lambda: dPre.mm(Wt))
    timeit("seq2col_bwd+res (T=1M,W=96)",
           lambda: hip.seq2col_bwd(dX3, starts, ends, dY))
    timeit("composed dX (T=1M,W=96)",
           lambda: hip.seq2col_bwd(dPre.mm(Wt), starts, ends, dY))
    timeit("mwe_bwd_dx (T=1M,W=96)",
           lambda: hip.mwe_bwd_dx(dPre, Wt, starts, ends, dY))
    # stage 1 + dX in one kernel: compare with the sum of the
    # mwe_bwd_stage1 and mwe_bwd_dx lines above
    timeit("mwe_bwd_fused (T=1M,W=96)",
           lambda: hip.mwe_bwd_fused(dY, dm, Mout, g, mu, rstd, which, Wt,
                                     starts, ends))


def bench_dpre():
    import numpy as np

    nF, HP, L = 13, 128, 20
    n_docs = 50000
    T = n_docs * L
    SS = 2 * T
    rng = np.random.default_rng(0)
    # doc-major feats: row r of doc d draws from doc d's tokens or pad
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), 2 * L)
    base = doc * L
    f = base[:, None] + rng.integers(0, L, (SS, nF))
    pad = rng.random((SS, nF)) < 0.25
    f[pad] = T
    feats = torch.from_numpy(f).to(dev)
    dS = torch.randn(SS, HP, device=dev, dtype=torch.bfloat16)
    # realistic sparsity: dSummed comes out of maxout_bwd — exactly one of
    # each piece pair (h, H+h) is nonzero
    pick = torch.randint(0, 2, (SS, 1, HP // 2), device=dev)
    dS.view(SS, 2, HP // 2).scatter_(1, pick, 0.0)
    dPre = torch.zeros(T + 1, nF, HP, device=dev, dtype=torch.bfloat16)
    timeit("dpre_scatter bf16 (1.9M rows)",
           lambda: hip.dpre_scatter(dS, feats, dPre, T))
    off = torch.arange(n_docs, device=dev, dtype=torch.int32) * L
    lens = torch.full((n_docs,), L, device=dev, dtype=torch.int32)
    dPre2 = torch.empty(T + 1, nF, HP, device=dev, dtype=torch.bfloat16)
    timeit("dpre_docmajor bf16 (1.9M rows)",
           lambda: hip.dpre_scatter_docmajor(dS, feats, dPre2, off, lens,
                                             T, 2, L))
    # diagnostics: atomic-op-rate hypothesis — nF=1 should be ~1/13 the
    # time if op-bound; fp32 (2x the ops of packed bf16) should be ~2x
    feats1 = feats[:, :1].contiguous()
    dPre1 = torch.zeros(T + 1, 1, HP, device=dev, dtype=torch.bfloat16)
    timeit("dpre_scatter bf16 nF=1",
           lambda: hip.dpre_scatter(dS, feats1, dPre1, T))
    dS32 = dS.float()
    dPre32 = torch.zeros(T + 1, nF, HP, device=dev, dtype=torch.float32)
    timeit("dpre_scatter fp32 (2x ops)",
           lambda: hip.dpre_scatter(dS32, feats, dPre32, T))


def bench_ce():
    SS, A = 2000000, 82
    scores = torch.randn(SS, A, device=dev, dtype=torch.bfloat16)
    valid = (torch.rand(SS, A, device=dev) < 0.5).to(torch.uint8)
    valid[:, 0] = 1
    gold = ((torch.rand(SS, A, device=dev) < 0.1).to(torch.uint8) & valid)
    timeit("transition_ce (2M rows, A=82)",
           lambda: hip.transition_ce(scores, gold, valid))


def bench_gpustate():
    n_docs, L, nL = 50000, 20, 40
    T = n_docs * L
    H, nF = 64, 13
    lens = torch.full((n_docs,), L, device=dev, dtype=torch.int32)
    off = (torch.arange(n_docs, device=dev, dtype=torch.int32) * L)
    pre = torch.randn(T + 1, nF, 2 * H, device=dev, dtype=torch.bfloat16)
    lowerB = torch.randn(2 * H, device=dev, dtype=torch.bfloat16)
    A = 2 + 2 * nL
    upperW = torch.randn(A, H, device=dev, dtype=torch.bfloat16)
    upperB = torch.randn(A, device=dev, dtype=torch.bfloat16)
    import numpy as np

    rng = np.random.default_rng(0)
    gh_np = np.zeros(T, dtype=np.int32)
    for d in range(n_docs):
        for i in range(1, L):
            gh_np[d * L + i] = rng.integers(0, i)
        gh_np[d * L] = -1
    gl_np = rng.integers(0, nL, T).astype(np.int32)
    tok_off = np.repeat(np.arange(n_docs, dtype=np.int64) * L, L)
    local = np.arange(T, dtype=np.int64) - tok_off
    ok = gh_np >= 0
    parent = tok_off[ok] + gh_np[ok]
    order = np.argsort(parent, kind="stable")
    kids_np = local[ok][order].astype(np.int32)
    kids_off_np = np.zeros(T + 1, dtype=np.int64)
    np.cumsum(np.bincount(parent, minlength=T), out=kids_off_np[1:])
    gh = torch.from_numpy(gh_np).to(dev)
    gl = torch.from_numpy(gl_np).to(dev)
    kids = torch.from_numpy(kids_np).to(dev)
    kids_off = torch.from_numpy(kids_off_np.astype(np.int32)).to(dev)
    timeit("gpu_arceager train (50k docs)",
           lambda: hip.gpu_arceager(pre, off, lens, gh, gl, kids_off, kids,
                                    lowerB, upperW, upperB, T, nL, True))
    # same shapes: compare against the train line plus transition_ce
    timeit("gpu_arceager train fused-CE (50k docs)",
           lambda: hip.gpu_arceager(pre, off, lens, gh, gl, kids_off, kids,
                                    lowerB, upperW, upperB, T, nL, True,
                                    fuse_ce=True))
    timeit("gpu_arceager decode (50k docs)",
           lambda: hip.gpu_arceager(pre, off, lens, gh, gl, kids_off, kids,
                                    lowerB, upperW, upperB, T, nL, False))
    A2 = 1 + 4 * 18
    pre6 = torch.randn(T + 1, 6, 2 * H, device=dev, dtype=torch.bfloat16)
    upW2 = torch.randn(A2, H, device=dev, dtype=torch.bfloat16)
    upB2 = torch.randn(A2, device=dev, dtype=torch.bfloat16)
    gold = torch.zeros(T, device=dev, dtype=torch.int32)
    timeit("gpu_biluo train (50k docs)",
           lambda: hip.gpu_biluo(pre6, off, lens, gold, lowerB, upW2, upB2,
                                 T, 18, True))
    timeit("gpu_biluo train fused-CE (50k docs)",
           lambda: hip.gpu_biluo(pre6, off, lens, gold, lowerB, upW2, upB2,
                                 T, 18, True, fuse_ce=True))


def bench_attn():
    """Fused flash-style MFMA attention vs SDPA flash at trf window shapes."""
    from spacy_ray_amd.ops.api import window_attention

    B, H, L, D = 1024, 12, 96, 64  # ~one bucket's worth of windows
    lens = torch.randint(20, L + 1, (B,), device=dev, dtype=torch.int32)
    q = torch.randn(B, H, L, D, device=dev, dtype=torch.bfloat16,
                    requires_grad=True)
    k = torch.randn_like(q, requires_grad=True)
    v = torch.randn_like(q, requires_grad=True)
    scale = D ** -0.5

    def fused_fb():
        out = window_attention(q, k, v, lens, scale, 0.1)
        out.sum().backward()
        q.grad = k.grad = v.grad = None

    timeit("attn fused fwd+bwd (1k win)", fused_fb)

    mask = (torch.arange(L, device=dev)[None, :] < lens[:, None]).view(B, 1, 1, L)

    def sdpa_fb():
        out = torch.nn.functional.scaled_dot_product_attention(
            q, k, v, attn_mask=mask, dropout_p=0.1, scale=scale)
        out.sum().backward()
        q.grad = k.grad = v.grad = None

    timeit("attn sdpa  fwd+bwd (1k win)", sdpa_fb)


def timeit_events(name, fn, iters=30, warmup=10):
    """Median and min of per-call GPU times (hip events around each call,
    after a warm-up that also settles the clocks)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    med = times[len(times) // 2]
    print(f"{name:40s} median {med:8.3f} ms  min {times[0]:8.3f} ms")
    return med


def bench_static_vectors():
    """static_vectors_fwd / static_vectors_bwd_dw against the composed path
    (index_select + mm, dY^T @ gathered) on the same inputs: T = 1M tokens,
    V = 20000, nM = 300 (table stride 320), Zipf-distributed rows with 5%
    out of vocabulary.  Both write / read the last column block of a
    [T, 5 nO] embed matrix, as MultiHashEmbed does."""
    import numpy as np

    T, V, nM, nMp = 1 << 20, 20000, 300, 320
    rng = np.random.default_rng(0)
    p = 1.0 / np.arange(1, V + 1)
    rows_np = rng.choice(V, size=T, p=p / p.sum()).astype(np.int32)
    rows_np[rng.random(T) < 0.05] = -1
    rows = torch.from_numpy(rows_np).to(dev)
    table = torch.zeros(V, nMp, device=dev, dtype=torch.bfloat16)
    table[:, :nM] = torch.randn(V, nM, device=dev) * 0.5
    oov = (rows < 0)[:, None]
    idx = rows.long().clamp(min=0)
    for nO in (96, 128):
        W = (torch.randn(nO, nM, device=dev) / nM ** 0.5).to(torch.bfloat16)
        X = torch.zeros(T, 5 * nO, device=dev, dtype=torch.bfloat16)
        dX = (torch.randn(T, 5 * nO, device=dev) * 0.1).to(torch.bfloat16)

        def composed_fwd():
            G = table.index_select(0, idx)[:, :nM].masked_fill(oov, 0)
            X[:, 4 * nO:] = G.mm(W.t())

        def composed_dw():
            G = table.index_select(0, idx)[:, :nM].masked_fill(oov, 0)
            return dX[:, 4 * nO:].t().mm(G)

        tag = f"(T=1M,nM=300,nO={nO})"
        timeit_events(f"static_vectors_fwd {tag}",
                      lambda: hip.static_vectors_fwd(table, rows, W, X, 4 * nO))
        timeit_events(f"composed fwd {tag}", composed_fwd)
        timeit_events(f"static_vectors_bwd_dw {tag}",
                      lambda: hip.static_vectors_bwd_dw(table, rows, dX, 4 * nO,
                                                        nO, 0, nM))
        timeit_events(f"composed dW {tag}", composed_dw)


def bench_hashembed():
    """MultiHashEmbed forward and backward, per-table path against the fused
    forward (multi_hashembed_fwd) and the token-sorted merged backward
    (hashembed_bwd_merged), sort and glue included on both sides.  T = 1M,
    W = 96, tables of 5000 / 2500 / 2500 / 2500 rows; Zipf ids over 5000
    types (the bench.py corpus) and over 100k types (real text: fewer
    tokens share an id, so fewer rows merge)."""
    import numpy as np

    T, W = 1 << 20, 96
    nrows = (5000, 2500, 2500, 2500)
    n = len(nrows)
    seeds = [1, 2, 3, 4]
    rng = np.random.default_rng(0)
    tables = [(torch.randn(R, W, device=dev) * 0.1).to(torch.bfloat16)
              for R in nrows]
    dX = (torch.randn(T, n * W, device=dev) * 0.1).to(torch.bfloat16)
    X = torch.empty(T, n * W, device=dev, dtype=torch.bfloat16)
    for n_types in (5000, 100000):
        p = 1.0 / np.arange(1, n_types + 1)
        cols = []
        for _ in range(n):
            types = rng.integers(1, 2 ** 62, n_types, dtype=np.int64)
            cols.append(types[rng.choice(n_types, size=T, p=p / p.sum())])
        ids4 = torch.from_numpy(np.stack(cols, axis=1)).to(dev)

        def fwd_old():
            return [hip.hashembed_fwd(t, ids4[:, i].contiguous(), seeds[i],
                                      X, i * W)[1]
                    for i, t in enumerate(tables)]

        def fwd_new():
            return hip.multi_hashembed_fwd(ids4, tables, seeds, X, 0)

        rows_old = fwd_old()
        rows_new, keys_new = fwd_new()

        def bwd_old():
            out = []
            for i, rows in enumerate(rows_old):
                dst = rows.reshape(-1)
                order = torch.argsort(dst)
                dst_sorted = dst[order].contiguous().int()
                src = (order // 4).int()
                dT32 = torch.zeros(nrows[i], W, dtype=torch.float32, device=dev)
                hip.seg_scatter_add(dst_sorted, src, dX[:, i * W:(i + 1) * W],
                                    dT32)
                out.append(dT32.to(torch.bfloat16))
            return out

        def bwd_new():
            out = []
            for i in range(n):
                order = torch.argsort(keys_new[i])
                dT32 = torch.zeros(nrows[i], W, dtype=torch.float32, device=dev)
                hip.hashembed_bwd_merged(order, rows_new[i],
                                         dX[:, i * W:(i + 1) * W], dT32)
                out.append(dT32.to(torch.bfloat16))
            return out

        def bwd_new_kernel_only(orders=[torch.argsort(k) for k in keys_new]):
            for i in range(n):
                dT32 = torch.zeros(nrows[i], W, dtype=torch.float32, device=dev)
                hip.hashembed_bwd_merged(orders[i], rows_new[i],
                                         dX[:, i * W:(i + 1) * W], dT32)

        tag = f"(T=1M,W=96,{n_types} types)"
        timeit_events(f"hashembed fwd x4 per-table {tag}", fwd_old)
        timeit_events(f"multi_hashembed_fwd {tag}", fwd_new)
        timeit_events(f"hashembed bwd x4 seg_scatter {tag}", bwd_old)
        timeit_events(f"hashembed bwd x4 merged {tag}", bwd_new)
        timeit_events(f"  merged kernels alone {tag}", bwd_new_kernel_only)


def _floret_lexicons(U):
    """Two lexicons of U distinct words: the synthetic corpus vocabulary
    (w0, w1, ...: short words, few n-grams) and pseudo-words whose lengths
    follow a real lexicon's (types are longer than tokens: 2..24 letters,
    mode 8)."""
    import numpy as np

    rng = np.random.default_rng(0)
    synthetic = [f"w{i}" for i in range(U)]
    lens = np.clip(rng.gamma(6.0, 1.5, size=U).round().astype(int), 2, 24)
    letters = np.array(list("etaoinshrdlucmfwypvbgkqjxz"))
    p = 1.0 / np.arange(1, 27)
    p /= p.sum()
    words, seen = [], set()
    for i, n in enumerate(lens.tolist()):
        w = "".join(rng.choice(letters, size=n, p=p))
        if w in seen:
            w += f"{i}"
        seen.add(w)
        words.append(w)
    return {"synthetic vocab": synthetic, "real-length words": words}


def bench_floret():
    """floret_words_mean against the composed torch path (index_select +
    segment sum + divide + cast) on the same inputs: R = 200000 rows, nM =
    300 (row stride 320), U = 50000 distinct words, minn = 4, maxn = 5,
    hash_count = 2.  The two paths alternate inside one timed loop.  Also
    prints the achieved read rate over the floor nnz * nMp * 2 bytes, the
    largest difference between the two results, and the host cost of
    building a 1M-token floret batch (dedupe + n-gram expansion)."""
    import numpy as np

    from spacy_ray_amd.ops import torch_ref as ref
    from spacy_ray_amd.vocab.vectors import Vectors

    R, nM, nMp, U = 200_000, 300, 320, 50_000
    rng = np.random.default_rng(0)
    vectors = Vectors(np.zeros((R, 1), dtype=np.float32), mode="floret",
                      minn=4, maxn=5, hash_count=2)
    table = torch.zeros(R, nMp, device=dev, dtype=torch.bfloat16)
    table[:, :nM] = torch.randn(R, nM, device=dev) * 0.5
    lexicons = _floret_lexicons(U)
    for tag, words in lexicons.items():
        offsets_np, idx_np = vectors.ngram_rows(words)
        nnz = int(idx_np.shape[0])
        counts = np.diff(offsets_np)
        offsets = torch.from_numpy(offsets_np).to(dev)
        idx = torch.from_numpy(idx_np).to(dev)
        out = torch.empty(U, nMp, device=dev, dtype=torch.bfloat16)
        print(f"floret {tag}: U = {U}, nnz = {nnz}, entries per word median "
              f"{int(np.median(counts))} max {int(counts.max())}")

        def fused():
            hip.floret_words_mean(table, offsets, idx, out)

        def composed():
            return ref.floret_words_mean(table, offsets, idx)

        fused()
        diff = (out.float() - composed().float()).abs().max().item()
        # alternate the two so that clock and cache state are shared
        for _ in range(10):
            fused()
            composed()
        torch.cuda.synchronize()
        times = {"fused": [], "composed": []}
        for _ in range(30):
            for name, fn in (("fused", fused), ("composed", composed)):
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
        floor_bytes = nnz * nMp * 2
        for name, ts in times.items():
            ts.sort()
            med = ts[len(ts) // 2]
            print(f"  floret_words_mean {name:9s} median {med:8.3f} ms  min "
                  f"{ts[0]:8.3f} ms  {floor_bytes / med / 1e9:8.3f} TB/s of "
                  f"row reads")
        print(f"  max |fused - composed| = {diff:.3e}")

    # host cost of one 1M-token floret batch, Zipf tokens over a 50k lexicon
    from spacy_ray_amd.models.batch import TokenBatch
    from spacy_ray_amd.vocab.doc import Doc, Vocab

    words = lexicons["real-length words"]
    vocab = Vocab("xx")
    vocab.vectors = vectors
    p = 1.0 / np.arange(1, U + 1)
    ids = rng.choice(U, size=1 << 20, p=p / p.sum())
    no_attrs = np.zeros((20, 4), dtype=np.uint64)  # not what is timed
    docs = [Doc(vocab, [words[i] for i in ids[k:k + 20]], attr_hashes=no_attrs)
            for k in range(0, 1 << 20, 20)]
    batch = TokenBatch(docs, "cpu")
    for d in docs:
        d.get_vector_keys("ORTH")  # per-Doc hashes are cached, as in training
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        inverse, offsets_np, idx_np, distinct = batch._build_floret("ORTH")
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    print(f"floret host batch build (T = {len(inverse)}, U = {len(distinct)}, "
          f"nnz = {len(idx_np)}): {best:.1f} ms (dedupe + n-gram expansion, "
          f"best of 3, token hashes cached per Doc)")


def bench_vecloss():
    """vectors_loss (srx_vecloss.hip.h) against the composed torch path
    (torch_ref.vectors_loss) on the same inputs: N = 150k masked tokens (15%
    of a 1M-word step), nM = 300 (table stride 320), V = 200k, Zipf rows
    with 5% out of vocabulary, both losses.  Both sides produce the row
    losses, their sum and dPred, as the forward of ops.vectors_loss does."""
    import numpy as np

    from spacy_ray_amd.ops import torch_ref as ref

    N, V, nM, nMp = 150_000, 200_000, 300, 320
    rng = np.random.default_rng(0)
    p = 1.0 / np.arange(1, V + 1)
    rows_np = rng.choice(V, size=N, p=p / p.sum()).astype(np.int32)
    rows_np[rng.random(N) < 0.05] = -1
    rows = torch.from_numpy(rows_np).to(dev)
    table = torch.zeros(V, nMp, device=dev, dtype=torch.bfloat16)
    table[:, :nM] = torch.randn(V, nM, device=dev) * 0.5
    pred = torch.randn(N, nM, device=dev).to(torch.bfloat16)
    row_loss = torch.empty(N, device=dev)
    dpred = torch.empty_like(pred)
    scale = 1.0 / N
    floor_bytes = N * (2 * nM * 2 + nMp * 2)
    for loss in ("cosine", "L2"):
        def fused():
            hip.vectors_loss(pred, table, rows, row_loss, dpred, loss == "L2",
                             scale)
            return row_loss.sum() * scale

        def composed():
            rl, dp = ref.vectors_loss(pred, table, rows, loss, scale)
            return rl.sum() * scale, dp

        lf = fused()
        lc, dc = composed()
        diff = (dpred.float() - dc.float()).abs().max().item()
        # alternate the two so that clock and cache state are shared
        for _ in range(10):
            fused()
            composed()
        torch.cuda.synchronize()
        times = {"fused": [], "composed": []}
        for _ in range(30):
            for name, fn in (("fused", fused), ("composed", composed)):
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
        print(f"vecloss {loss} (N={N}, nM={nM}, V={V}):")
        for name, ts in times.items():
            ts.sort()
            med = ts[len(ts) // 2]
            print(f"  vectors_loss {name:9s} median {med:8.3f} ms  min "
                  f"{ts[0]:8.3f} ms  {floor_bytes / med / 1e9:8.3f} TB/s of the "
                  f"floor bytes")
        print(f"  loss fused {float(lf):.6f} composed {float(lc):.6f}, "
              f"max |dPred fused - composed| = {diff:.3e}")


def bench_mixer():
    """Fused mixer (mixer_fwd / mixer_bwd_fused + dW) against the composed
    chain (linear_cdw -> maxout -> layernorm -> * mask and its autograd
    backward), forward and backward, T = 1M, W = 96, NS = 4, with mask.  The
    two paths alternate in one loop; median of 30 event-timed calls after 10
    warm-ups.  Bytes: the fused forward reads E and the mask and writes Y,
    Mout and which; the fused backward kernel reads dY, the mask, Mout and
    which and writes dPre and dE (its dW GEMM is timed with it, as the
    composed backward's is)."""
    from spacy_ray_amd.ops import api as ops

    T, W, NS = 1 << 20, 96, 4
    bf = torch.bfloat16
    E = (torch.randn(T, NS * W, device=dev) * 0.5).to(bf).requires_grad_(True)
    Wm = (torch.randn(3 * W, NS * W, device=dev) / (NS * W) ** 0.5).to(bf) \
        .requires_grad_(True)
    bias = torch.zeros(3 * W, device=dev, dtype=bf, requires_grad=True)
    g = torch.ones(W, device=dev, dtype=bf, requires_grad=True)
    b = torch.zeros(W, device=dev, dtype=bf, requires_grad=True)
    mask = ops.dropout_mask_like(torch.empty(T, W, device=dev, dtype=bf), 0.1)
    dY = torch.randn(T, W, device=dev).to(bf)
    leaves = (E, Wm, bias, g, b)

    def fused():
        return ops.mixer_layer(E, Wm, bias, g, b, mask, 1e-5)

    def composed():
        Y = ops.linear_cdw(E, Wm, bias)
        Y = ops.maxout(Y.view(T, 3, W))
        return ops.layernorm(Y, g, b, 1e-5) * mask

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    ts = {(n, d): [] for n in ("fused", "composed") for d in ("fwd", "bwd")}
    for it in range(40):
        for name, fn in (("fused", fused), ("composed", composed)):
            t_f, Y = timed(fn)
            t_b, _ = timed(lambda: torch.autograd.grad(Y, leaves, dY))
            if it >= 10:
                ts[name, "fwd"].append(t_f)
                ts[name, "bwd"].append(t_b)
    fwd_bytes = T * (NS * W * 2 + W * 2 + 2 * W * 2 + W)
    bwd_bytes = T * (2 * W * 2 + W * 2 + W + 3 * W * 2 + NS * W * 2)
    for d, nbytes in (("fwd", fwd_bytes), ("bwd", bwd_bytes)):
        for name in ("fused", "composed"):
            v = sorted(ts[name, d])
            med = v[len(v) // 2]
            extra = ""
            if name == "fused":
                extra = (f"  {nbytes / 1e9:.2f} GB -> {nbytes / med / 1e9:.2f} "
                         f"TB/s" + (" (incl. dW GEMM time)" if d == "bwd" else ""))
            print(f"  mixer {d} {name:9s} median {med:7.3f} ms  min {v[0]:7.3f} "
                  f"max {v[-1]:7.3f}{extra}")


def bench_mwe_dw():
    """MWE backward, dW path: old = full mwe_bwd_fused (writes dPre [T, 3W]) +
    seq2col_fwd + mm_dw_chunked; new = compact mwe_bwd_fused (writes dM
    [T, W]) + mwe_bwd_dw.  T = 1M, W = 96, with mask, docs of 20 tokens.  The
    two paths alternate in one loop; median (min) of 30 event-timed calls
    after 10 warm-ups, each piece timed on its own as well.  Bytes of
    mwe_bwd_dw: dM + which + X + the boundary bytes (the 505 MB floor)."""
    from spacy_ray_amd import _srx_hip as hip
    from spacy_ray_amd.ops import api as ops

    T, W = 1 << 20, 96
    bf = torch.bfloat16
    X = (torch.randn(T, W, device=dev) * 0.5).to(bf)
    Wt = (torch.randn(3 * W, 3 * W, device=dev) / (3 * W) ** 0.5).to(bf)
    bias = torch.zeros(3 * W, device=dev, dtype=bf)
    g = torch.ones(W, device=dev, dtype=bf)
    b = torch.zeros(W, device=dev, dtype=bf)
    lens = torch.full((T // 20 + 1,), 20, device=dev, dtype=torch.long)
    lens[-1] = T - 20 * (T // 20)
    starts, ends = ops.boundary_masks_u8(lens, T)
    mask = ops.dropout_mask_like(torch.empty(T, W, device=dev, dtype=bf), 0.1)
    _, Mout, which, mu, rstd = hip.mwe_layer_fwd(X, Wt, bias, g, b, starts, ends,
                                                 mask, 1e-5)
    dY = torch.randn(T, W, device=dev).to(bf)

    def fused_full():
        return hip.mwe_bwd_fused(dY, mask, Mout, g, mu, rstd, which, Wt, starts,
                                 ends)

    def fused_compact():
        return hip.mwe_bwd_fused(dY, mask, Mout, g, mu, rstd, which, Wt, starts,
                                 ends, compact=True)

    dPre = fused_full()[0]
    dM = fused_compact()[0]
    X3 = hip.seq2col_fwd(X, starts, ends)
    pieces = {
        "old: mwe_bwd_fused (dPre)": fused_full,
        "old: seq2col_fwd": lambda: hip.seq2col_fwd(X, starts, ends),
        "old: mm_dw_chunked": lambda: ops.mm_dw_chunked(dPre, X3),
        "old: total": lambda: ops.mm_dw_chunked(
            fused_full()[0], hip.seq2col_fwd(X, starts, ends)),
        "new: mwe_bwd_fused (dM)": fused_compact,
        "new: mwe_bwd_dw": lambda: hip.mwe_bwd_dw(dM, which, X, starts, ends),
        "new: total": lambda: hip.mwe_bwd_dw(fused_compact()[0], which, X, starts,
                                             ends),
    }
    ts = {k: [] for k in pieces}
    for it in range(40):
        for name, fn in pieces.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= 10:
                ts[name].append(e0.elapsed_time(e1))
    dw_bytes = T * (2 * W * 2 + W + 2)
    for name, v in ts.items():
        v = sorted(v)
        med = v[len(v) // 2]
        extra = ""
        if name == "new: mwe_bwd_dw":
            extra = (f"  {dw_bytes / 1e6:.0f} MB -> {dw_bytes / med / 1e9:.2f} TB/s"
                     " (incl. the partial reduction)")
        print(f"  mwe_dw {name:28s} median {med:7.3f} ms  min {v[0]:7.3f} "
              f"max {v[-1]:7.3f}{extra}")
    a = pieces["old: total"]().float()
    c = pieces["new: total"]().float()
    print(f"  mwe_dw max |old - new| {float((a - c).abs().max()):.3e} at max |dW| "
          f"{float(c.abs().max()):.3e}")


ALL = {"mwe": bench_mwe, "dpre": bench_dpre, "ce": bench_ce, "mixer": bench_mixer,
       "mwe_dw": bench_mwe_dw,
       "floret": bench_floret, "vecloss": bench_vecloss,
       "gpustate": bench_gpustate, "attn": bench_attn,
       "static_vectors": bench_static_vectors,
       "hashembed": bench_hashembed}

if __name__ == "__main__":
    names = sys.argv[1:] or list(ALL)
    for n in names:
        ALL[n]()
