"""Nearest neighbours and vector pruning on the CPU: the composed
torch_ref.vectors_most_similar against float64, Vectors.most_similar /
pruned, Vocab.prune_vectors and `init vectors --prune`."""
import numpy as np
import pytest
import torch

from spacy_ray_amd.ops import api as ops
from spacy_ray_amd.ops import torch_ref as ref
from spacy_ray_amd.pipeline.language import check_static_vectors_config, init_vectors
from spacy_ray_amd.vocab.doc import Vocab
from spacy_ray_amd.vocab.vectors import Vectors, load_vectors_dir

KEPT, DROPPED, DIM = 12, 30, 20
SRC = (5 * np.arange(DROPPED)) % KEPT  # the kept row each dropped row is near
WORDS = [f"w{i}" for i in range(KEPT + DROPPED)]


def _data():
    rng = np.random.default_rng(5)
    kept = rng.standard_normal((KEPT, DIM)).astype(np.float32)
    noise = 0.05 * rng.standard_normal((DROPPED, DIM)).astype(np.float32)
    return np.concatenate([kept, kept[SRC] + noise])


def _write_word2vec(path, data):
    lines = [f"{len(data)} {data.shape[1]}"]
    lines += [w + " " + " ".join(repr(float(x)) for x in v) for w, v in zip(WORDS, data)]
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.parametrize("n", (1, 4))
def test_composed_path_against_float64_with_ties(n, monkeypatch):
    gen = torch.Generator().manual_seed(3)
    t = torch.randn(40, 7, generator=gen)
    t[30] = t[4]   # a duplicate row: the lower index wins
    t[9] = 0       # a zero row scores 0
    q = torch.randn(11, 7, generator=gen)
    q[0] = t[4]
    q[1] = 0       # a zero query: every score 0, rows 0..n-1
    unit = lambda x: x.double() / x.double().norm(dim=1, keepdim=True).clamp(min=1e-300)
    sims = (unit(q) @ unit(t).t()).clamp(-1, 1)
    want_s, want_r = (-sims).sort(dim=1, stable=True)
    rows, scores = ref.vectors_most_similar(q, t, n, batch_size=4)
    assert rows.dtype == torch.int32 and rows.shape == scores.shape == (11, n)
    assert torch.equal(rows[1].long(), torch.arange(n)) and (scores[1] == 0).all()
    assert rows[0, 0] == 4
    if n > 1:
        assert rows[0, 1] == 30
    assert torch.equal(rows[2:].long(), want_r[2:, :n])
    assert (scores.double() + want_s[:, :n]).abs().max() < 1e-6
    monkeypatch.setenv("SRX_MOST_SIMILAR", "fused")  # CPU: composed anyway
    assert torch.equal(ops.vectors_most_similar(q, t, n)[0], rows)
    assert not ops.vectors_most_similar_available(q, t, n)
    monkeypatch.setenv("SRX_MOST_SIMILAR", "bogus")
    with pytest.raises(ValueError, match="SRX_MOST_SIMILAR"):
        ops.vectors_most_similar(q, t, n)
    with pytest.raises(ValueError, match="outside 1..40"):
        ref.vectors_most_similar(q, t, 41)


def test_vectors_most_similar_shapes_keys_and_errors():
    data = _data()
    vectors = Vectors.from_words(WORDS[:KEPT], data[:KEPT])
    keys, rows, scores = vectors.most_similar(data[KEPT:], n=3, batch_size=7,
                                              device="cpu")
    assert keys.shape == rows.shape == scores.shape == (DROPPED, 3)
    assert (keys.dtype, rows.dtype, scores.dtype) == (np.uint64, np.int32, np.float32)
    assert (rows[:, 0] == SRC).all()
    assert (scores[:, 0] > 0.9).all() and (np.diff(scores, axis=1) <= 0).all()
    assert (vectors.find_rows(keys.reshape(-1)) == rows.reshape(-1)).all()
    # two keys on one row: the first in sorted-key order is reported; a row
    # without a key reports 0
    shared = Vectors(data[:3], vectors.keys[:4], np.array([0, 1, 1, 0]))
    keys, rows, _ = shared.most_similar(data[:3], device="cpu")
    assert rows[:, 0].tolist() == [0, 1, 2]
    assert keys[:, 0].tolist() == [int(shared.keys[0]), int(shared.keys[1]), 0]
    for n in (0, 13):
        with pytest.raises(ValueError, match="outside 1..12"):
            vectors.most_similar(data[:2], n=n)
    with pytest.raises(ValueError, match="queries must be"):
        vectors.most_similar(data[:2, :5])
    floret = Vectors(data, mode="floret", minn=3, maxn=4)
    with pytest.raises(ValueError, match="floret vectors have no word-to-row map"):
        floret.most_similar(data[:2])
    vocab = Vocab()
    vocab.vectors = floret
    with pytest.raises(ValueError, match="floret"):
        vocab.prune_vectors(3)


def test_pruned_and_prune_vectors(tmp_path):
    vocab = Vocab("en")
    vocab.strings.add_batch(WORDS)
    old = vocab.vectors = Vectors.from_words(WORDS, _data(), name="toy")
    new, new_rows, scores = old.pruned(KEPT, device="cpu")
    want_rows = np.concatenate([np.arange(KEPT), SRC])
    assert new.shape == (KEPT, DIM) and np.array_equal(new.data, old.data[:KEPT])
    assert np.array_equal(new.keys, old.keys)
    assert (new.find_words(WORDS) == want_rows).all()
    assert (new_rows == new.rows).all()
    kept = old.rows < KEPT
    assert (scores[kept] == 1).all() and ((scores[~kept] > 0.9) & (scores[~kept] < 1)).all()

    remap = vocab.prune_vectors(KEPT)
    assert vocab.vectors.shape == (KEPT, DIM)
    assert set(remap) == set(WORDS[KEPT:])
    for i, word in enumerate(WORDS[KEPT:]):
        syn, score = remap[word]
        cos = np.dot(old.data[KEPT + i], old.data[SRC[i]]) / (
            np.linalg.norm(old.data[KEPT + i]) * np.linalg.norm(old.data[SRC[i]]))
        assert syn == WORDS[SRC[i]] and abs(score - cos) < 1e-5
    assert np.array_equal(vocab.get_vector(WORDS[KEPT + 3]), old.data[SRC[3]])
    vocab.vectors.to_disk(tmp_path)
    again = Vectors.from_disk(tmp_path)
    assert again.shape == (KEPT, DIM) and (again.find_words(WORDS) == want_rows).all()
    # nothing to prune
    assert vocab.prune_vectors(KEPT) == {} and vocab.prune_vectors(100) == {}
    assert vocab.vectors.shape == (KEPT, DIM)
    same, rows, _ = old.pruned(len(old))
    assert same is old and np.array_equal(rows, old.rows)


def test_init_vectors_prune(tmp_path):
    from typer.testing import CliRunner

    from spacy_ray_amd.cli.main import app

    src = tmp_path / "vectors.txt"
    _write_word2vec(src, _data())
    want_rows = np.concatenate([np.arange(KEPT), SRC])
    nlp = init_vectors("en", src, tmp_path / "api", prune=KEPT)
    assert nlp.vocab.vectors.shape == (KEPT, DIM)
    r = CliRunner().invoke(app, ["init", "vectors", "en", str(src),
                                 str(tmp_path / "cli"), "--prune", str(KEPT)])
    assert r.exit_code == 0, r.output
    assert f"shape=({KEPT}, {DIM})" in r.output and f"keys={len(WORDS)}" in r.output
    for out in ("api", "cli"):
        v = load_vectors_dir(tmp_path / out)
        assert v.shape == (KEPT, DIM) and (v.find_words(WORDS) == want_rows).all()
        lines = check_static_vectors_config({"initialize": {"vectors": str(tmp_path / out)}})
        assert lines and lines[0].startswith("vectors OK")
    nlp = init_vectors("en", src, tmp_path / "t", truncate=32, prune=KEPT)  # truncate first
    assert len(nlp.vocab.vectors.keys) == 32 and nlp.vocab.vectors.shape == (KEPT, DIM)
    r = CliRunner().invoke(app, ["init", "vectors", "en", str(src), str(tmp_path / "f"),
                                 "--mode", "floret", "--prune", "5"])
    assert r.exit_code != 0 and "--prune cannot be used with --mode floret" in r.output
