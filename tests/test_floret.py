"""Floret vectors on the CPU: n-gram rows against an independent pure-Python
implementation, the `.floret` reader, serialisation, `init vectors --mode
floret`, Doc.vector and the TokenBatch dedupe / composed forward."""
import gzip
import json

import numpy as np
import pytest
import torch

from spacy_ray_amd.models.batch import TokenBatch
from spacy_ray_amd.vocab.doc import Doc, Vocab
from spacy_ray_amd.vocab.vectors import (
    Vectors, load_vectors_dir, read_floret_text)

M64 = (1 << 64) - 1


# ------------------------------------------- independent reference (Python)
def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _fmix(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def murmur3_x64_128(data: bytes, seed: int):
    """MurmurHash3 x64_128 -> the 16 output bytes as four little-endian
    uint32."""
    c1, c2 = 0x87c37b91114253d5, 0x4cf5ad432745937f
    h1 = h2 = seed
    n = len(data)
    for b in range(n // 16):
        k1 = int.from_bytes(data[16 * b:16 * b + 8], "little")
        k2 = int.from_bytes(data[16 * b + 8:16 * b + 16], "little")
        k1 = (_rotl((k1 * c1) & M64, 31) * c2) & M64
        h1 ^= k1
        h1 = ((_rotl(h1, 27) + h2) * 5 + 0x52dce729) & M64
        k2 = (_rotl((k2 * c2) & M64, 33) * c1) & M64
        h2 ^= k2
        h2 = ((_rotl(h2, 31) + h1) * 5 + 0x38495ab5) & M64
    tail = data[16 * (n // 16):]
    if len(tail) > 8:
        k2 = int.from_bytes(tail[8:], "little")
        h2 ^= (_rotl((k2 * c2) & M64, 33) * c1) & M64
    if tail:
        k1 = int.from_bytes(tail[:8], "little")
        h1 ^= (_rotl((k1 * c1) & M64, 31) * c2) & M64
    h1 ^= n
    h2 ^= n
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    h1, h2 = _fmix(h1), _fmix(h2)
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    out = h1.to_bytes(8, "little") + h2.to_bytes(8, "little")
    return [int.from_bytes(out[4 * i:4 * i + 4], "little") for i in range(4)]


def ref_ngrams(word, minn, maxn, bow="<", eow=">"):
    if not word:
        return []
    padded = bow + word + eow          # a str: slices are by code point
    grams = [padded]
    for n in range(minn, maxn + 1):
        for i in range(len(padded) - n + 1):
            grams.append(padded[i:i + n])
    return grams


def ref_rows(words, nrows, minn, maxn, hash_count, hash_seed, bow="<", eow=">"):
    offsets, idx = [0], []
    for w in words:
        for g in ref_ngrams(w, minn, maxn, bow, eow):
            h = murmur3_x64_128(g.encode("utf8"), hash_seed)
            idx.extend(x % nrows for x in h[:hash_count])
        offsets.append(len(idx))
    return offsets, idx


def test_reference_murmur_matches_the_string_store_hash():
    """The test's own murmur3 against the one the project already ships
    (hash_utf8 = first 8 output bytes at seed 1), over every tail length."""
    from spacy_ray_amd.vocab.vectors import hash_words

    words = ["x" * n for n in range(1, 40)] + ["żółw", "日本語"]
    got = hash_words(words)
    for w, g in zip(words, got):
        h = murmur3_x64_128(w.encode("utf8"), 1)
        assert int(g) == h[0] | (h[1] << 32)


# ------------------------------------------------------------- n-gram rows
# minn = 4, maxn = 5: "a" is shorter than minn (padded length 3), "ab" has
# padded length == minn, "abc" == maxn; the rest are ASCII and multi-byte
WORDS = ["hello", "a", "ab", "abc", "Tokenization", "żółw", "日本語",
         "\U0001F600", "x\U0001F600y", "", "it's"]


def _table(nrows=97, dim=10, seed=0):
    return np.random.default_rng(seed).standard_normal((nrows, dim)).astype("f")


@pytest.mark.parametrize("hash_count,hash_seed", [(1, 0), (2, 0), (4, 0), (2, 2166136261)])
def test_ngram_rows_match_the_python_reference(hash_count, hash_seed):
    v = Vectors(_table(), mode="floret", minn=4, maxn=5, hash_count=hash_count,
                hash_seed=hash_seed)
    offsets, idx = v.ngram_rows(WORDS)
    assert offsets.dtype == np.int32 and idx.dtype == np.int32
    want_off, want_idx = ref_rows(WORDS, 97, 4, 5, hash_count, hash_seed)
    assert offsets.tolist() == want_off
    assert idx.tolist() == want_idx
    assert idx.min() >= 0 and idx.max() < 97


def test_ngram_counts_and_whole_form_listed_twice():
    v = Vectors(_table(), mode="floret", minn=4, maxn=5, hash_count=1)
    offsets, idx = v.ngram_rows(WORDS)
    counts = dict(zip(WORDS, np.diff(offsets).tolist()))
    assert counts[""] == 0
    assert counts["a"] == 1                 # "<a>" only: shorter than minn
    assert counts["ab"] == 2                # "<ab>" as itself and as its 4-gram
    assert counts["abc"] == 1 + 2 + 1       # whole, two 4-grams, the 5-gram
    assert counts["hello"] == 1 + 4 + 3     # padded length 7
    # n-grams are by code point: 3 code points each, 9 and 4 bytes
    assert counts["日本語"] == counts["abc"]
    assert counts["\U0001F600"] == counts["a"]
    assert counts["x\U0001F600y"] == counts["abc"]
    for w in ("ab", "abc"):
        i = WORDS.index(w)
        rows = idx[offsets[i]:offsets[i + 1]]
        assert rows[0] == rows[-1]          # no de-duplication
    # other markers change the strings that are hashed
    v2 = Vectors(_table(), mode="floret", minn=4, maxn=5, bow="[", eow="]")
    assert v2.ngram_rows(["hello"])[1].tolist() == ref_rows(
        ["hello"], 97, 4, 5, 1, 0, "[", "]")[1]


def test_get_batch_is_the_mean_of_the_ngram_rows():
    data = _table(dim=7)
    v = Vectors(data, mode="floret", minn=3, maxn=5, hash_count=2, hash_seed=7)
    got = v.get_batch(WORDS)
    assert got.shape == (len(WORDS), 7) and got.dtype == np.float32
    offsets, idx = v.ngram_rows(WORDS)
    for i, w in enumerate(WORDS):
        rows = idx[offsets[i]:offsets[i + 1]]
        want = (data[rows].astype(np.float64).mean(axis=0) if len(rows)
                else np.zeros(7))
        # fp32 sum of n values and one divide
        tol = 2 * max(len(rows), 1) * 2.0 ** -24 * np.abs(data).max()
        assert np.abs(got[i] - want).max() <= tol, w
    assert not got[WORDS.index("")].any()
    assert v.get_batch([]).shape == (0, 7)
    assert v.get_batch(["", ""]).shape == (2, 7)


def test_constructor_validates_the_settings():
    data = _table()
    for kw in (dict(minn=0, maxn=3), dict(minn=4, maxn=3), dict(minn=0, maxn=0)):
        with pytest.raises(ValueError, match="minn"):
            Vectors(data, mode="floret", **kw)
    for hc in (0, 5):
        with pytest.raises(ValueError, match="hash_count"):
            Vectors(data, mode="floret", minn=3, maxn=4, hash_count=hc)
    with pytest.raises(ValueError, match="mode"):
        Vectors(data, mode="fasttext", minn=3, maxn=4)
    with pytest.raises(ValueError, match="only the hash of NORM is kept"):
        Vectors(data, mode="floret", minn=3, maxn=4, key_attr="NORM")
    v = Vectors(data, mode="floret", minn=3, maxn=4, key_attr="LOWER")
    assert v.is_floret and len(v.keys) == 0 and len(v.rows) == 0
    assert v.shape == (97, 10)


def test_find_rows_raises_in_floret_mode():
    v = Vectors(_table(), mode="floret", minn=3, maxn=4)
    with pytest.raises(ValueError, match="no word-to-row map"):
        v.find_rows(np.zeros(2, dtype=np.uint64))
    with pytest.raises(ValueError, match="no word-to-row map"):
        v.find_words(["a"])
    default = Vectors.from_words(["a"], np.ones((1, 3), dtype="f"))
    assert not default.is_floret
    with pytest.raises(ValueError, match="floret"):
        default.ngram_rows(["a"])


# ------------------------------------------------------------------ reader
def _write_floret(path, data, order=None, header="4 5 2 11 < >", gz=False):
    order = list(range(len(data))) if order is None else order
    lines = [f"{len(data)} {data.shape[1]} {header}"]
    for r in order:
        lines.append(f"{r} " + " ".join(repr(float(x)) for x in data[r]))
    text = "\n".join(lines) + "\n"
    if gz:
        with gzip.open(path, "wt", encoding="utf8") as f:
            f.write(text)
    else:
        path.write_text(text, encoding="utf8")
    return lines


@pytest.mark.parametrize("gz", [False, True])
def test_read_floret_text_round_trip_rows_out_of_order(tmp_path, gz):
    data = _table(nrows=13, dim=4)
    order = np.random.default_rng(3).permutation(13).tolist()
    src = tmp_path / ("v.floret.gz" if gz else "v.floret")
    _write_floret(src, data, order=order, gz=gz)
    got, settings = read_floret_text(src)
    assert np.array_equal(got, data)
    assert settings == {"minn": 4, "maxn": 5, "hash_count": 2, "hash_seed": 11,
                        "bow": "<", "eow": ">"}


def test_read_floret_text_malformed_input(tmp_path):
    data = _table(nrows=6, dim=3)
    src = tmp_path / "v.floret"

    def rewrite(mutate):
        lines = _write_floret(src, data)
        mutate(lines)
        src.write_text("\n".join(lines) + "\n", encoding="utf8")

    def setline(i, text):
        return lambda lines: lines.__setitem__(i, text)

    rewrite(setline(0, "6 3 4 5 2 11 <"))                  # seven fields
    with pytest.raises(ValueError, match=r"v\.floret: line 1: expected the floret header"):
        read_floret_text(src)
    rewrite(setline(0, "6 3 four 5 2 11 < >"))
    with pytest.raises(ValueError, match=r"line 1: .*integers"):
        read_floret_text(src)
    rewrite(setline(0, "0 3 4 5 2 11 < >"))
    with pytest.raises(ValueError, match=r"line 1: .*positive"):
        read_floret_text(src)
    rewrite(setline(3, "2 1.0 2.0"))                       # too few floats
    with pytest.raises(ValueError, match=r"line 4: expected a row index and 3 floats"):
        read_floret_text(src)
    rewrite(setline(3, "2 1.0 x 3.0"))
    with pytest.raises(ValueError, match=r"line 4: vector values must be floats"):
        read_floret_text(src)
    rewrite(setline(3, "two 1.0 2.0 3.0"))
    with pytest.raises(ValueError, match=r"line 4: the row index must be an integer"):
        read_floret_text(src)
    rewrite(setline(3, "6 1.0 2.0 3.0"))                   # rows are 0..5
    with pytest.raises(ValueError, match=r"line 4: row index 6 outside 0\.\.5"):
        read_floret_text(src)
    rewrite(setline(3, "1 1.0 2.0 3.0"))                   # row 1 again, 2 missing
    with pytest.raises(ValueError, match=r"line 4: row index 1 appears twice"):
        read_floret_text(src)
    rewrite(lambda lines: lines.pop(3))
    with pytest.raises(ValueError, match=r"1 of 6 rows are missing \(first: 2\)"):
        read_floret_text(src)
    src.write_text("", encoding="utf8")
    with pytest.raises(ValueError, match="no floret header"):
        read_floret_text(src)


# --------------------------------------------------- serialisation and CLI
def test_to_disk_from_disk_round_trip(tmp_path):
    data = _table()
    v = Vectors(data, mode="floret", minn=3, maxn=6, hash_count=3,
                hash_seed=99, bow="[", eow="]", key_attr="LOWER", name="toy")
    v.to_disk(tmp_path / "vocab")
    meta = json.loads((tmp_path / "vocab" / "vectors.json").read_text())
    assert meta == {"name": "toy", "shape": [97, 10], "key_attr": "LOWER",
                    "mode": "floret", "minn": 3, "maxn": 6, "hash_count": 3,
                    "hash_seed": 99, "bow": "[", "eow": "]"}
    back = Vectors.from_disk(tmp_path / "vocab")
    assert back.is_floret and back.name == "toy" and back.key_attr == "LOWER"
    assert back.floret_settings() == v.floret_settings()
    assert np.array_equal(back.data, data)
    assert np.array_equal(back.get_batch(WORDS), v.get_batch(WORDS))


def test_default_mode_directory_still_loads(tmp_path):
    """The files a default-mode table has always written: no `mode` key."""
    from safetensors.numpy import save_file

    from spacy_ray_amd.vocab.vectors import hash_words

    data = _table(nrows=3, dim=4)
    keys = hash_words(["a", "b", "c"])
    vocab_dir = tmp_path / "vocab"
    vocab_dir.mkdir()
    save_file({"data": data, "keys": keys.view(np.int64),
               "rows": np.arange(3, dtype=np.int32)},
              str(vocab_dir / "vectors.safetensors"))
    (vocab_dir / "vectors.json").write_text(json.dumps(
        {"name": "old", "shape": [3, 4], "key_attr": "ORTH"}))
    v = Vectors.from_disk(vocab_dir)
    assert v.mode == "default" and not v.is_floret
    assert v.find_words(["c", "zz"]).tolist() == [2, -1]
    # and default mode still writes exactly that
    v.to_disk(tmp_path / "again")
    assert json.loads((tmp_path / "again" / "vectors.json").read_text()) == {
        "name": "old", "shape": [3, 4], "key_attr": "ORTH"}


def test_init_vectors_mode_floret_through_the_cli(tmp_path):
    from typer.testing import CliRunner

    from spacy_ray_amd.cli.main import app

    data = _table(nrows=31, dim=5)
    src = tmp_path / "v.floret"
    _write_floret(src, data, order=list(range(30, -1, -1)))
    out = tmp_path / "out"
    r = CliRunner().invoke(app, ["init", "vectors", "fi", str(src), str(out),
                                 "--mode", "floret", "--name", "toy"])
    assert r.exit_code == 0, r.output
    assert "mode='floret'" in r.output
    v = load_vectors_dir(out)
    assert v.is_floret and v.name == "toy" and v.shape == (31, 5)
    assert v.floret_settings() == {"minn": 4, "maxn": 5, "hash_count": 2,
                                   "hash_seed": 11, "bow": "<", "eow": ">"}
    assert np.array_equal(v.data, data)
    # a word2vec file under --mode floret is an error with a line number
    bad = tmp_path / "w2v.txt"
    bad.write_text("2 5\na 1 2 3 4 5\nb 1 2 3 4 5\n")
    r = CliRunner().invoke(app, ["init", "vectors", "fi", str(bad),
                                 str(tmp_path / "o2"), "--mode", "floret"])
    assert r.exit_code != 0 and "line 1" in r.output
    r = CliRunner().invoke(app, ["init", "vectors", "fi", str(src),
                                 str(tmp_path / "o3"), "--mode", "nope"])
    assert r.exit_code != 0 and "--mode" in r.output


# ----------------------------------------------------------- Doc and config
def _floret_vocab(key_attr="ORTH", dim=6, nrows=211):
    vocab = Vocab("xx")
    vocab.vectors = Vectors(_table(nrows=nrows, dim=dim, seed=5), mode="floret",
                            minn=3, maxn=5, hash_count=2, key_attr=key_attr)
    return vocab


def test_doc_vector_for_words_in_no_lexicon():
    vocab = _floret_vocab()
    doc = Doc(vocab, ["qwrtzx", "", "blorptangle"])
    vec = doc.vector
    assert vec.shape == (6,) and np.abs(vec).max() > 0
    want = vocab.vectors.get_batch(["qwrtzx", "blorptangle"]).mean(axis=0)
    assert np.allclose(vec, want, rtol=0, atol=1e-6)
    assert vocab.has_vector("qwrtzx") and not vocab.has_vector("")
    assert np.array_equal(vocab.get_vector("qwrtzx"),
                          vocab.vectors.get_batch(["qwrtzx"])[0])
    assert doc.similarity(Doc(vocab, ["qwrtzx", "blorptangle"])) > 0.999
    assert not Doc(vocab, [""]).vector.any()
    with pytest.raises(ValueError, match="get_floret_table"):
        doc.get_vector_rows()
    # LOWER keys hash the lower-cased string
    low = _floret_vocab("LOWER")
    assert np.array_equal(Doc(low, ["QwRtZx"]).vector, Doc(low, ["qwrtzx"]).vector)
    assert not np.array_equal(Doc(vocab, ["QwRtZx"]).vector,
                              Doc(vocab, ["qwrtzx"]).vector)


def test_norm_key_attr_is_rejected_everywhere(tmp_path):
    from spacy_ray_amd.models.layers import StaticVectors
    from spacy_ray_amd.pipeline.language import check_static_vectors_config

    vocab = _floret_vocab()
    with pytest.raises(ValueError, match="only the hash of NORM is kept"):
        StaticVectors(8, 6, key_attr="NORM", vectors=vocab.vectors)
    sv = StaticVectors(8, 6, key_attr="NORM")
    with pytest.raises(ValueError, match="only the hash of NORM is kept"):
        sv.bind(vocab.vectors)
    # debug config: a floret directory reports its mode; one whose json was
    # edited to NORM is reported as unsupported
    vec_dir = tmp_path / "vec"
    vocab.vectors.to_disk(vec_dir / "vocab")
    lines = check_static_vectors_config({"initialize": {"vectors": str(vec_dir)}})
    assert any("floret" in line for line in lines)
    meta_path = vec_dir / "vocab" / "vectors.json"
    meta = json.loads(meta_path.read_text())
    meta["key_attr"] = "NORM"
    meta_path.write_text(json.dumps(meta))
    with pytest.raises(ValueError, match="only the hash of NORM is kept"):
        check_static_vectors_config({"initialize": {"vectors": str(vec_dir)}})


# ------------------------------------------------------------------- Batch
DOCS = [["The", "cat", "sat", "", "the", "Cat"],
        [],
        ["żółw", "sat", "日本語", "The", "żółw"],
        ["", "neverseen"]]


@pytest.mark.parametrize("key_attr", ["ORTH", "LOWER"])
@pytest.mark.parametrize("pad_to", [1, 16])
def test_batch_dedupe_and_csr(key_attr, pad_to):
    vocab = _floret_vocab(key_attr)
    vocab.vector_key_attrs.append(key_attr)
    docs = [Doc(vocab, w) for w in DOCS]
    batch = TokenBatch(docs, "cpu", pad_to=pad_to)
    assert batch.vec_rows is None
    assert ("floret", key_attr) in batch.staged   # built at construction
    inverse, offsets, idx = batch.get_floret(key_attr)
    assert all(t.dtype == torch.int32 for t in (inverse, offsets, idx))
    assert inverse.shape == (batch.n_tokens,)
    _, _, _, words = batch._build_floret(key_attr)
    flat = [w for d in DOCS for w in d]
    keyed = [w.lower() if key_attr == "LOWER" else w for w in flat]
    distinct = {w for w in keyed if w}
    U = offsets.numel() - 1
    assert U == len(distinct) == len(words) and set(words) == distinct
    assert U == (8 if key_attr == "ORTH" else 6)
    for t, w in enumerate(keyed):
        if w:
            assert words[inverse[t]] == w
        else:
            assert inverse[t] == -1
    assert (inverse[len(flat):] == -1).all()      # the pad pseudo-doc
    assert batch.n_tokens == (16 if pad_to == 16 else len(flat))
    want_off, want_idx = vocab.vectors.ngram_rows(words)
    assert offsets.tolist() == want_off.tolist()
    assert idx.tolist() == want_idx.tolist()
    # the temporary table: computed once, shared
    t1, inv1 = batch.get_floret_table(vocab.vectors, key_attr, "cpu", torch.float32)
    t2, _ = batch.get_floret_table(vocab.vectors, key_attr, "cpu", torch.float32)
    assert t1 is t2 and inv1 is inverse
    assert t1.shape == (U, 6) and not t1.requires_grad


def test_dedupe_keys_first_occurrence_order():
    from spacy_ray_amd import _srx_cpu

    keys = np.array([7, 3, 7, 0, 9, 3, 0, 7], dtype=np.uint64)
    inverse, first = _srx_cpu.dedupe_keys(keys, 0)
    assert inverse.dtype == np.int32 and first.dtype == np.int64
    assert inverse.tolist() == [0, 1, 0, -1, 2, 1, -1, 0]
    assert first.tolist() == [0, 1, 4]
    rng = np.random.default_rng(0)
    big = rng.integers(1, 5000, 200000).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    inverse, first = _srx_cpu.dedupe_keys(big, 0)
    uniq, idx0 = np.unique(big, return_index=True)
    assert len(first) == len(uniq)
    assert np.array_equal(np.sort(first), np.sort(idx0))
    assert np.array_equal(big[first][inverse], big)
    empty_inv, empty_first = _srx_cpu.dedupe_keys(np.zeros(0, np.uint64), 0)
    assert empty_inv.shape == (0,) and empty_first.shape == (0,)


@pytest.mark.parametrize("fuse_into_embed", [False, True])
def test_composed_forward_on_cpu(fuse_into_embed):
    """StaticVectors / MultiHashEmbed over a floret batch on the CPU equal
    get_batch(words) @ W.T within fp32 rounding."""
    from spacy_ray_amd.models.layers import StaticVectors
    from spacy_ray_amd.models.tok2vec import MultiHashEmbed

    torch.manual_seed(0)
    vocab = _floret_vocab("ORTH")
    vocab.vector_key_attrs.append("ORTH")
    docs = [Doc(vocab, w) for w in DOCS]
    batch = TokenBatch(docs, "cpu", pad_to=16)
    flat = [w for d in DOCS for w in d]
    G = np.zeros((batch.n_tokens, 6), dtype=np.float64)
    G[:len(flat)] = vocab.vectors.get_batch(flat)
    if fuse_into_embed:
        embed = MultiHashEmbed(8, rows=[20, 10, 10, 10],
                               include_static_vectors=True, vocab=vocab)
        W = embed.static_vectors.W
        X = ops_multi(embed, batch)
        got = X[:, 4 * 8:]
    else:
        sv = StaticVectors(8, 6, key_attr="ORTH", vectors=vocab.vectors)
        W = sv.W
        got = sv(batch)
    want = G @ W.detach().double().numpy().T
    # fp32: the mean (n <= 32 terms) and a 6-term dot product
    tol = 64 * 2.0 ** -24 * np.abs(G).max() * float(W.detach().abs().max()) * 6
    assert np.abs(got.detach().double().numpy() - want).max() <= tol
    assert not got[len(flat):].any()
    assert not got[flat.index("")].any()
    got.sum().backward()
    assert W.grad is not None and torch.isfinite(W.grad).all()
    assert W.grad.abs().max() > 0


def ops_multi(embed, batch):
    from spacy_ray_amd.ops import api as ops

    sv = embed.static_vectors
    return ops.multi_hashembed(batch.attr_ids, embed.seeds, list(embed.tables),
                               (*sv.table_and_rows(batch), sv.W))


def test_ref_floret_words_mean_guards():
    """The composed op: empty slices give zero rows, entries outside the
    table contribute nothing."""
    from spacy_ray_amd.ops import api as ops

    table = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    offsets = torch.tensor([0, 2, 2, 5], dtype=torch.int32)
    idx = torch.tensor([0, 3, 1, 4, -1], dtype=torch.int32)
    out = ops.floret_words_mean(table, offsets, idx)
    assert out.shape == (3, 3)
    assert torch.equal(out[0], (table[0] + table[3]) / 2)
    assert not out[1].any()
    assert torch.equal(out[2], table[1] / 3)
    assert ops.floret_words_mean(table, offsets[:1], idx[:0]).shape == (0, 3)
