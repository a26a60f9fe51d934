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


def _docmajor_case(nF, cap_mult, n_docs=50000, L=20, HP=128):
    """Doc-major arenas as the GPU state machines lay them out: doc d owns
    rows [cap_mult*d*L, cap_mult*(d+1)*L), each feature a token of doc d or
    (a quarter of them) the pad row; dSummed with the maxout zero pattern."""
    import numpy as np

    T = n_docs * L
    SS = cap_mult * T
    rng = np.random.default_rng(0)
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), cap_mult * L)
    f = (doc * L)[:, None] + rng.integers(0, L, (SS, nF))
    f[rng.random((SS, nF)) < 0.25] = T
    feats = torch.from_numpy(f).to(dev)
    dS = torch.randn(SS, HP, device=dev, dtype=torch.bfloat16)
    pick = torch.randint(0, 2, (SS, 1, HP // 2), device=dev)
    dS.view(SS, 2, HP // 2).scatter_(1, pick, 0.0)
    off = torch.arange(n_docs, device=dev, dtype=torch.int32) * L
    lens = torch.full((n_docs,), L, device=dev, dtype=torch.int32)
    return T, dS, feats, off, lens


def bench_dpre():
    """torch.zeros + dpre_scatter (packed-bf16 atomics) against torch.empty +
    dpre_gather (one wave per doc, plain stores) on the same doc-major
    inputs, at the parser shape (nF = 13, cap_mult = 2) and the NER shape
    (nF = 6, cap_mult = 1): 1M tokens in 20-word docs, HP = 128, bf16.  The
    two alternate in one loop; median (min) of 30 event-timed calls after 10
    warm-ups.  Floor bytes of the gather: dSummed and feats read once, dPre
    written once."""
    L, HP = 20, 128
    for label, nF, cap_mult in (("parser", 13, 2), ("NER", 6, 1)):
        T, dS, feats, off, lens = _docmajor_case(nF, cap_mult, L=L, HP=HP)
        SS = feats.shape[0]

        def atomic():
            dPre = torch.zeros(T + 1, nF, HP, device=dev, dtype=torch.bfloat16)
            return hip.dpre_scatter(dS, feats, dPre, T)

        def gather():
            dPre = torch.empty(T + 1, nF, HP, device=dev, dtype=torch.bfloat16)
            return hip.dpre_gather(dS, feats, dPre, off, lens, T, cap_mult, L, T)

        floor = SS * HP * 2 + SS * nF * 8 + T * nF * HP * 2
        res = _alternate({"zeros + dpre_scatter": atomic,
                          "empty + dpre_gather": gather})
        print(f"dpre {label} (T={T}, rows={SS}, nF={nF}, HP={HP}, bf16):")
        for name, (med, mn) in res.items():
            print(f"  {name:22s} median {med:8.3f} ms  min {mn:8.3f} ms  "
                  f"{floor / med / 1e9:6.3f} TB/s of the {floor / 1e9:.2f} GB "
                  f"gather floor")
    # diagnostics of the atomic kernel: nF=1 should be ~1/13 the time if
    # op-bound; fp32 (2x the ops of packed bf16) should be ~2x
    T, dS, feats, off, lens = _docmajor_case(13, 2, L=L, HP=HP)
    feats1 = feats[:, :1].contiguous()
    dPre1 = torch.zeros(T + 1, 1, HP, device=dev, dtype=torch.bfloat16)
    timeit("dpre_scatter bf16 nF=1",
           lambda: hip.dpre_scatter(dS, feats1, dPre1, T))
    dS32 = dS.float()
    dPre32 = torch.zeros(T + 1, 13, HP, device=dev, dtype=torch.float32)
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


def bench_most_similar():
    """vectors_most_similar (srx_vecsim.hip.h) against the composed path
    (torch_ref.vectors_most_similar in bf16, batch 1024) on the same inputs,
    nM = 300 (row stride 320).  Pruning shape: nQ = 200k queries, V = 20k
    rows, n = 1.  Interactive shape: nQ = 1, V = 1M, n = 8, with the
    launcher's split count and with splits = 1.  The composed path is also
    timed with torch.topk in place of the stable sort (no tie order, so not
    the same contract, but the cheapest composed form).  The fused path is
    timed with its inv(t) pre-pass and, as Vectors.most_similar calls it,
    with the cached vectors_row_inv(table).  The paths alternate in one loop; median
    of 30 event-timed calls after 10 warm-ups."""
    from spacy_ray_amd.ops import api as ops
    from spacy_ray_amd.ops import torch_ref as ref

    vs = ops.hip_vecsim_ext()
    assert vs is not None, "_srx_hip_vecsim is not built"
    nM, nMp = 300, 320

    def composed_topk(q, t, n):
        unit = lambda x: x / x.float().norm(dim=1, keepdim=True).clamp_(min=1e-30).to(x.dtype)
        tn = unit(t).t()
        out = [unit(q[i:i + 1024]).mm(tn).topk(n, dim=1) for i in range(0, len(q), 1024)]
        return torch.cat([o.indices for o in out]), torch.cat([o.values for o in out])

    for label, nQ, V, n, split_list in (("pruning", 200_000, 20_000, 1, (0,)),
                                        ("interactive", 1, 1_000_000, 8, (0, 1))):
        table = torch.zeros(V, nMp, device=dev, dtype=torch.bfloat16)
        table[:, :nM] = torch.randn(V, nM, device=dev) * 0.5
        q = torch.zeros(nQ, nMp, device=dev, dtype=torch.bfloat16)
        q[:, :nM] = torch.randn(nQ, nM, device=dev) * 0.5
        inv = vs.vectors_row_inv(table)
        fns = {f"fused splits={s}": (lambda s=s: vs.vectors_most_similar(q, table, n, s))
               for s in split_list}
        fns["fused, cached inv"] = lambda: vs.vectors_most_similar(q, table, n, 0, inv)
        fns["composed sort"] = lambda: ref.vectors_most_similar(q, table, n, 1024)
        fns["composed topk"] = lambda: composed_topk(q, table, n)
        rows_f = fns[f"fused splits={split_list[0]}"]()[0]
        rows_c = fns["composed sort"]()[0]
        agree = (rows_f[:, 0] == rows_c[:, 0]).float().mean().item()
        for _ in range(10):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(30):
            for name, fn in fns.items():
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
        flops = 2.0 * nQ * V * nMp
        print(f"most_similar {label} (nQ={nQ}, V={V}, nM={nM}, n={n}): top-1 rows "
              f"fused == composed on {agree:.4f} of the queries; similarity matrix "
              f"of the composed path: {nQ * V * 2 * 2 / 1e9:.3f} GB written + read "
              f"in bf16 ({nQ * V * 4 * 2 / 1e9:.3f} GB in fp32)")
        for name, ts in times.items():
            ts.sort()
            med = ts[len(ts) // 2]
            print(f"  {name:18s} median {med:9.3f} ms  min {ts[0]:9.3f} ms  "
                  f"{flops / med / 1e9:8.1f} TFLOP/s  "
                  f"{V * nMp * 2 / med / 1e9:6.3f} TB/s of one table pass")


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


def bench_mwe_wide():
    """One MWE block at W = 256 (srx_mwe_wide.hip.h), forward and backward
    including dW, fused (ops.mwe_layer) against the composed route of
    MaxoutWindowEncoder (seq2col -> linear_cdw -> maxout -> layernorm ->
    F.dropout -> residual and its autograd backward) on the same inputs, docs
    of 20 tokens, dropout 0.1.  T = 256K and, if memory allows, 1M.  The two
    routes alternate in one loop; median / min / max of 30 event-timed calls
    after 10 warm-ups, so the spread of each route is on its line."""
    from spacy_ray_amd.ops import api as ops

    W = 256
    bf = torch.bfloat16
    for T in (1 << 18, 1 << 20):
        try:
            X = (torch.randn(T, W, device=dev) * 0.5).to(bf).requires_grad_(True)
            Wt = (torch.randn(3 * W, 3 * W, device=dev) / (3 * W) ** 0.5).to(bf) \
                .requires_grad_(True)
            bias = torch.zeros(3 * W, device=dev, dtype=bf, requires_grad=True)
            g = torch.ones(W, device=dev, dtype=bf, requires_grad=True)
            b = torch.zeros(W, device=dev, dtype=bf, requires_grad=True)
            lens = torch.full((T // 20 + 1,), 20, device=dev, dtype=torch.long)
            lens[-1] = T - 20 * (T // 20)
            starts, ends = ops.boundary_masks_u8(lens, T)
            mask = ops.dropout_mask_like(torch.empty(T, W, device=dev, dtype=bf), 0.1)
            dY = torch.randn(T, W, device=dev).to(bf)
            leaves = (X, Wt, bias, g, b)

            def fused():
                return ops.mwe_layer(X, Wt, bias, g, b, starts, ends, mask, 1e-5)

            def composed():
                Y = ops.linear_cdw(ops.seq2col(X, lens, starts, ends), Wt, bias)
                Y = ops.layernorm(ops.maxout(Y.view(T, 3, W)), g, b, 1e-5)
                return X + torch.nn.functional.dropout(Y, 0.1)

            def timed(fn):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), out

            ts = {(n, d): [] for n in ("fused", "composed")
                  for d in ("fwd", "bwd+dW", "total")}
            for it in range(40):
                for name, fn in (("fused", fused), ("composed", composed)):
                    t_f, Y = timed(fn)
                    t_b, _ = timed(lambda: torch.autograd.grad(Y, leaves, dY))
                    del Y
                    if it >= 10:
                        ts[name, "fwd"].append(t_f)
                        ts[name, "bwd+dW"].append(t_b)
                        ts[name, "total"].append(t_f + t_b)
        except torch.OutOfMemoryError:
            print(f"  mwe_wide T={T}: out of memory, skipped")
            continue
        flops = 2.0 * T * (3 * W) * (3 * W)
        for d in ("fwd", "bwd+dW", "total"):
            for name in ("fused", "composed"):
                v = sorted(ts[name, d])
                med = v[len(v) // 2]
                nf = {"fwd": 1, "bwd+dW": 2, "total": 3}[d]
                print(f"  mwe_wide T={T} {d:6s} {name:9s} median {med:8.3f} ms  "
                      f"min {v[0]:8.3f}  max {v[-1]:8.3f}  "
                      f"{nf * flops / med / 1e9:7.1f} TFLOP/s")


def _alternate(fns, iters=30, warmup=10):
    """Median (and min) per-call GPU time of each fn, the fns alternating in
    one loop so that clock and cache state are shared."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    out = {}
    for name, ts in times.items():
        ts.sort()
        out[name] = (ts[len(ts) // 2], ts[0])
    return out


def bench_span_pool():
    """span_pool (srx_spanpool.hip.h) against the composed path
    (torch_ref.span_pool and its autograd backward) on the same inputs: T =
    1,048,576 tokens in 20-word docs, W = 96, bf16, every 1..3-gram a span.
    Forward and backward are timed separately; then the spancat reducer
    head's scores + BCE loss, forward + backward, with both routes."""
    import numpy as np

    from spacy_ray_amd.ops import api as ops
    from spacy_ray_amd.ops import torch_ref as ref
    from spacy_ray_amd.pipeline.pipes import SpancatReducerHead

    T, W, doc = 1 << 20, 96, 20
    starts, ends = [], []
    for off in range(0, T, doc):
        n = min(doc, T - off)
        for k in (1, 2, 3):
            a = np.arange(off, off + max(0, n - k + 1))
            starts.append(a)
            ends.append(a + k)
    starts, ends = np.concatenate(starts), np.concatenate(ends)
    index = ops.span_index(starts, ends, T, dev)
    S = index.n_spans
    rows = (S + 63) // 64 * 64
    X = torch.randn(T, W, device=dev).to(torch.bfloat16)
    dR = torch.randn(rows, 4 * W, device=dev).to(torch.bfloat16)
    fwd_bytes = S * (4 * W * 2 + W) + T * W * 2
    bwd_bytes = S * 4 * W * 2 + S * W + T * W * 2
    print(f"span_pool (T={T}, W={W}, bf16, S={S} spans of 1..3 tokens):")

    Rf, which = hip.span_pool_fwd(X, index.starts, index.ends, rows)
    fwd = _alternate({
        "fused": lambda: hip.span_pool_fwd(X, index.starts, index.ends, rows),
        "composed": lambda: ref.span_pool(X, index.starts, index.ends, 3),
    })
    for name, (med, mn) in fwd.items():
        print(f"  fwd {name:9s} median {med:8.3f} ms  min {mn:8.3f} ms  "
              f"{fwd_bytes / med / 1e9:8.3f} TB/s of the {fwd_bytes} floor bytes")

    x = X.clone().requires_grad_(True)
    Rc, _ = ref.span_pool(x, index.starts, index.ends, 3)

    def composed_bwd():
        return torch.autograd.grad(Rc, x, dR[:S], retain_graph=True)[0]

    def fused_bwd():
        return hip.span_pool_bwd(dR, which, index.starts, index.ends,
                                 index.tok_offsets, index.tok_spans)

    diff = (fused_bwd().float() - composed_bwd().float()).abs().max().item()
    bwd = _alternate({"fused": fused_bwd, "composed": composed_bwd})
    for name, (med, mn) in bwd.items():
        print(f"  bwd {name:9s} median {med:8.3f} ms  min {mn:8.3f} ms  "
              f"{bwd_bytes / med / 1e9:8.3f} TB/s of the {bwd_bytes} floor bytes")
    print(f"  max |R fused - composed| = "
          f"{(Rf[:S].float() - Rc.float()).abs().max().item():.3e}, "
          f"max |dX fused - composed| = {diff:.3e}")
    del Rc, x, Rf

    head = SpancatReducerHead(W, W, 4).to(dev).to(torch.bfloat16)
    target = (torch.rand(S, 4, device=dev) < 0.05).float()
    t2v = X.clone().requires_grad_(True)

    def step(span_pool, mixer):
        def run():
            os.environ["SRX_SPAN_POOL"] = span_pool
            os.environ["SRX_MIXER"] = mixer
            scores = head(t2v, index)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(
                scores.float(), target, reduction="sum") / S
            loss.backward()
            t2v.grad = None
            head.zero_grad(set_to_none=True)
        return run

    routes = _alternate({"fused": step("fused", ""),
                         "composed": step("composed", "composed")}, iters=10, warmup=3)
    os.environ.pop("SRX_SPAN_POOL")
    os.environ.pop("SRX_MIXER")
    for name, (med, mn) in routes.items():
        print(f"  head + loss fwd+bwd {name:9s} median {med:8.3f} ms  min {mn:8.3f} ms")


def bench_attention_pool():
    """attention_pool (srx_attnpool.hip.h) against the composed path
    (torch_ref.attention_pool and its autograd backward) on the same inputs:
    T = 1,048,576 tokens as 20-token and as 400-token docs, bf16, W = 96 and
    768, without keys (the ensemble) and, at W = 96, with keys (parametric
    attention).  Forward and backward are timed separately, whole calls."""
    from spacy_ray_amd.ops import torch_ref as ref

    T = 1 << 20
    for W, doc, keys in ((96, 20, False), (96, 400, False), (96, 20, True),
                         (768, 20, False), (768, 400, False)):
        bounds = list(range(0, T, doc)) + [T]
        offsets = torch.tensor(bounds, dtype=torch.int32, device=dev)
        D = len(bounds) - 1
        X = torch.randn(T, W, device=dev).to(torch.bfloat16)
        K = torch.randn(T, W, device=dev).to(torch.bfloat16) if keys else None
        q = torch.randn(W, device=dev) / W ** 0.5
        dP = torch.randn(D, W, device=dev).to(torch.bfloat16)
        rw = 2 if keys else 1
        fwd_bytes = rw * T * W * 2 + D * W * 6
        bwd_bytes = 2 * rw * T * W * 2 + D * W * 6
        print(f"attention_pool (T={T}, W={W}, bf16, {D} docs of {doc} tokens, "
              f"keys={keys}):")

        P, P32, lse, uo = hip.attention_pool_fwd(X, K, offsets, q, D)
        fwd = _alternate({
            "fused": lambda: hip.attention_pool_fwd(X, K, offsets, q, D),
            "composed": lambda: ref.attention_pool(X, offsets, q, K),
        })
        for name, (med, mn) in fwd.items():
            print(f"  fwd {name:9s} median {med:8.3f} ms  min {mn:8.3f} ms  "
                  f"{fwd_bytes / med / 1e9:8.3f} TB/s of the {fwd_bytes} floor bytes")

        ins = [t.clone().requires_grad_(True) for t in ((X, q, K) if keys else (X, q))]
        Pc = ref.attention_pool(ins[0], offsets, ins[1], ins[2] if keys else None)

        def composed_bwd():
            return torch.autograd.grad(Pc, ins, dP, retain_graph=True)

        def fused_bwd():
            return hip.attention_pool_bwd(X, K, offsets, uo, q, dP, P32, lse)

        diff = (fused_bwd()[0].float() - composed_bwd()[0].float()).abs().max().item()
        bwd = _alternate({"fused": fused_bwd, "composed": composed_bwd})
        for name, (med, mn) in bwd.items():
            print(f"  bwd {name:9s} median {med:8.3f} ms  min {mn:8.3f} ms  "
                  f"{bwd_bytes / med / 1e9:8.3f} TB/s of the {bwd_bytes} floor bytes")
        print(f"  max |P fused - composed| = "
              f"{(P.float() - Pc.float()).abs().max().item():.3e}, "
              f"max |dX fused - composed| = {diff:.3e}")
        del Pc, ins, X, K, P, P32


def bench_sparse_linear():
    """sparse_linear (srx_sparselinear.hip.h) against the composed path
    (ops.ngram_buckets + torch_ref.sparse_linear and its autograd backward)
    on the bench corpus's shape: 50,000 docs of 20 tokens, Zipf ids over 5000
    types, G = 3, L = 262144, bf16, nO = 4 and 32.  Whole calls: the fused
    backward includes the keys kernel, the sort, the dWeight zero fill and
    the fix-up; the sort is also timed alone."""
    import numpy as np

    from spacy_ray_amd.ops import api as ops
    from spacy_ray_amd.ops import torch_ref as ref

    D, doc, G, L = 50000, 20, 3, 262144
    rng = np.random.RandomState(0)
    p = 1.0 / np.arange(1, 5001)
    types = rng.randint(1, 2 ** 62, 5000).astype(np.int64)
    ids = torch.from_numpy(types[rng.choice(5000, D * doc, p=p / p.sum())]).to(dev)
    offsets = torch.arange(0, D * doc + 1, doc, dtype=torch.int32, device=dev)
    nnz = D * sum(doc - n + 1 for n in range(1, G + 1))
    for nO in (4, 32):
        W = torch.randn(L, nO, device=dev).to(torch.bfloat16)
        bias = torch.randn(nO, device=dev)
        dS = torch.randn(D, nO, device=dev)
        # floors: forward = one table row per entry, the ids, the scores;
        # backward = the 2 G T keys written and read once (the sort's own
        # traffic is not counted), dScores once, dWeight written
        fwd_bytes = 2 * nnz * nO * 2 + D * doc * 8 + D * nO * 4
        bwd_bytes = 2 * G * D * doc * 8 * 2 + D * nO * 4 + L * nO * 2
        print(f"sparse_linear (D={D}, T={D * doc}, G={G}, L={L}, bf16, nO={nO}, "
              f"{2 * nnz} entries):")

        def composed_fwd(w=W):
            buckets = ops.ngram_buckets(ids, offsets, G, L)
            return ref.sparse_linear(ids, offsets, w, bias, G, buckets)

        fwd = _alternate({
            "fused": lambda: hip.sparse_linear_fwd(ids, offsets, W, bias, G),
            "composed": composed_fwd,
        })
        for name, (med, mn) in fwd.items():
            print(f"  fwd {name:9s} median {med:8.3f} ms  min {mn:8.3f} ms  "
                  f"{fwd_bytes / med / 1e9:8.3f} TB/s of the {fwd_bytes} floor bytes")

        w = W.clone().requires_grad_(True)
        Sc = composed_fwd(w)

        def composed_bwd():
            return torch.autograd.grad(Sc, w, dS, retain_graph=True)[0]

        def fused_bwd():
            keys = hip.sparse_linear_keys(ids, offsets, G, L)
            return hip.sparse_linear_bwd(torch.sort(keys).values, dS, L, True)

        keys = hip.sparse_linear_keys(ids, offsets, G, L)
        diff = (fused_bwd().float() - composed_bwd().float()).abs().max().item()
        bwd = _alternate({"fused": fused_bwd, "composed": composed_bwd,
                          "sort": lambda: torch.sort(keys).values})
        for name, (med, mn) in bwd.items():
            print(f"  bwd {name:9s} median {med:8.3f} ms  min {mn:8.3f} ms  "
                  f"{bwd_bytes / med / 1e9:8.3f} TB/s of the {bwd_bytes} floor bytes")
        print(f"  sort share of the fused backward: "
              f"{bwd['sort'][0] / bwd['fused'][0]:.2f}")
        Sf = hip.sparse_linear_fwd(ids, offsets, W, bias, G)
        print(f"  max |scores fused - composed| = "
              f"{(Sf - Sc.detach()).abs().max().item():.3e}, "
              f"max |dW fused - composed| = {diff:.3e}")
        del Sc, w


def bench_char_embed():
    """char_embed_fwd / char_embed_bwd (srx_charembed.hip.h) against the
    composed path (advanced indexing, index_add_) on the same inputs: T =
    1,048,576 tokens, nC = 8, nM = 64, bf16; ids letter-heavy (Zipf over 26
    letters, a few other bytes) with about a third of the cells 255.  Both
    sides write / read the first column block of a [T, nC nM + 96] embed
    matrix; the composed forward's copy into the block stands for its cat.
    Then the whole op, forward + backward, both routes."""
    import numpy as np

    from spacy_ray_amd.ops import api as ops
    from spacy_ray_amd.ops import torch_ref as ref

    T, nC, nM, W = 1 << 20, 8, 64, 96
    rng = np.random.default_rng(0)
    p = 1.0 / np.arange(1, 27)
    ids_np = 97 + rng.choice(26, size=(T, nC), p=p / p.sum())
    other = rng.random((T, nC))
    ids_np[other < 0.05] = rng.integers(0, 255, size=int((other < 0.05).sum()))
    ids_np[rng.random((T, nC)) < 0.33] = 255
    ids = torch.from_numpy(ids_np.astype(np.uint8)).to(dev)
    E = (torch.randn(nC, 256, nM, device=dev) * 0.1).to(torch.bfloat16)
    X = torch.zeros(T, nC * nM + W, device=dev, dtype=torch.bfloat16)
    dX = (torch.randn(T, nC * nM + W, device=dev) * 0.1).to(torch.bfloat16)
    block = dX[:, :nC * nM]
    S, per = hip.char_embed_slices(T, nC)
    io_bytes = T * nC * (nM * 2 + 1)
    print(f"char_embed (T={T}, nC={nC}, nM={nM}, bf16, "
          f"{float((ids == 255).float().mean()):.2f} of the cells 255, "
          f"S={S} slices of {per} tokens):")

    def composed_fwd():
        X[:, :nC * nM] = ref.char_embed_forward(E, ids)

    fwd = _alternate({"fused": lambda: hip.char_embed_fwd(E, ids, X, 0),
                      "composed": composed_fwd})
    for name, (med, mn) in fwd.items():
        print(f"  fwd {name:9s} median {med:8.3f} ms  min {mn:8.3f} ms  "
              f"{io_bytes / med / 1e9:8.3f} TB/s of the {io_bytes} floor bytes")
    bwd = _alternate({
        "fused": lambda: hip.char_embed_bwd(block, ids, nC, nM, False),
        "determin.": lambda: hip.char_embed_bwd(block, ids, nC, nM, True),
        "composed": lambda: ref.char_embed_backward(block, ids, nC, nM),
    })
    for name, (med, mn) in bwd.items():
        print(f"  bwd {name:9s} median {med:8.3f} ms  min {mn:8.3f} ms  "
              f"{io_bytes / med / 1e9:8.3f} TB/s of the {io_bytes} floor bytes")
    diff = (hip.char_embed_bwd(block, ids, nC, nM, False).float()
            - ref.char_embed_backward(block, ids, nC, nM).float()).abs().max().item()
    print(f"  max |dE fused - composed| = {diff:.3e}")

    table = (torch.randn(5000, W, device=dev) * 0.1).to(torch.bfloat16).requires_grad_(True)
    Ep = E.clone().requires_grad_(True)
    hash_ids = torch.from_numpy(rng.integers(1, 2 ** 62, size=(T, 4))).to(dev)[:, 0]

    def step(mode):
        def run():
            os.environ["SRX_CHAR_EMBED"] = mode
            ops.char_embed(Ep, ids, table, hash_ids, 5).backward(dX)
            Ep.grad = table.grad = None
        return run

    routes = _alternate({"fused": step("fused"), "composed": step("composed")},
                        iters=10, warmup=3)
    os.environ.pop("SRX_CHAR_EMBED")
    for name, (med, mn) in routes.items():
        print(f"  op fwd+bwd {name:9s} median {med:8.3f} ms  min {mn:8.3f} ms")


ALL = {"mwe": bench_mwe, "sparse_linear": bench_sparse_linear, "dpre": bench_dpre, "ce": bench_ce, "mixer": bench_mixer,
       "mwe_dw": bench_mwe_dw, "mwe_wide": bench_mwe_wide,
       "floret": bench_floret, "vecloss": bench_vecloss,
       "most_similar": bench_most_similar, "span_pool": bench_span_pool, "attention_pool": bench_attention_pool,
       "gpustate": bench_gpustate, "attn": bench_attn,
       "static_vectors": bench_static_vectors,
       "hashembed": bench_hashembed, "char_embed": bench_char_embed}

if __name__ == "__main__":
    names = sys.argv[1:] or list(ALL)
    for n in names:
        ALL[n]()
