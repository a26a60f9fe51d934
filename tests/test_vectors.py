"""Static word vectors on the CPU: the Vectors table, `init vectors`,
serialisation, the StaticVectors layer and its reference ops."""
import gzip
import json

import numpy as np
import pytest
import torch

from spacy_ray_amd.config.config import Config
from spacy_ray_amd.pipeline.language import (
    check_static_vectors_config, init_nlp, init_vectors)
from spacy_ray_amd.vocab.doc import Doc, Example, Vocab
from spacy_ray_amd.vocab.vectors import Vectors, load_vectors_dir

WORDS = [f"Word{i}" if i % 5 == 0 else f"word{i}" for i in range(50)]


def _write_txt(path, words, data, header=True, gz=False):
    lines = [f"{len(words)} {data.shape[1]}"] if header else []
    for w, v in zip(words, data):
        lines.append(w + " " + " ".join(repr(float(x)) for x in v))
    text = "\n".join(lines) + "\n"
    if gz:
        with gzip.open(path, "wt", encoding="utf8") as f:
            f.write(text)
    else:
        path.write_text(text, encoding="utf8")


@pytest.fixture(scope="module")
def table():
    return np.random.default_rng(0).standard_normal((50, 12)).astype(np.float32)


# ------------------------------------------------------------ init vectors
@pytest.mark.parametrize("header,gz", [(True, False), (False, True)])
def test_init_vectors_gives_a_loadable_directory(tmp_path, table, header, gz):
    src = tmp_path / ("v.txt.gz" if gz else "v.txt")
    _write_txt(src, WORDS, table, header=header, gz=gz)
    init_vectors("en", src, tmp_path / "out", name="toy")
    vectors = load_vectors_dir(tmp_path / "out")
    assert vectors.shape == (50, 12) and vectors.name == "toy"
    assert np.array_equal(vectors.data, table)
    rows = vectors.find_words(["word3", "Word0", "nope", "word49", "word0"])
    assert rows.dtype == np.int32
    assert rows.tolist() == [3, 0, -1, 49, -1]
    meta = json.loads((tmp_path / "out" / "vocab" / "vectors.json").read_text())
    assert meta == {"name": "toy", "shape": [50, 12], "key_attr": "ORTH"}
    # the directory is a pipeline: an empty one loads it back
    from spacy_ray_amd.pipeline.language import build_nlp

    nlp = build_nlp(Config.from_disk(tmp_path / "out" / "config.cfg"))
    nlp.from_disk(tmp_path / "out")
    assert nlp.vocab.has_vector("word3") and not nlp.vocab.has_vector("nope")
    assert np.array_equal(nlp.vocab.get_vector("word3"), table[3])


def test_init_vectors_truncate(tmp_path, table):
    src = tmp_path / "v.txt"
    _write_txt(src, WORDS, table)
    nlp = init_vectors("en", src, tmp_path / "out", truncate=10)
    assert nlp.vocab.vectors.shape == (10, 12)
    assert nlp.vocab.vectors.find_words(["word9", "Word10"]).tolist() == [9, -1]


def test_init_vectors_rejects_a_malformed_line_with_its_number(tmp_path, table):
    src = tmp_path / "v.txt"
    _write_txt(src, WORDS, table)
    lines = src.read_text().split("\n")
    lines[7] = "broken 1.0 2.0"          # line 8 of the file: too few floats
    src.write_text("\n".join(lines))
    with pytest.raises(ValueError, match=r"line 8\b"):
        init_vectors("en", src, tmp_path / "out")
    lines[7] = "broken " + " ".join(["x"] * 12)
    src.write_text("\n".join(lines))
    with pytest.raises(ValueError, match=r"line 8\b"):
        init_vectors("en", src, tmp_path / "out")


def test_find_rows_shared_rows_and_empty():
    from spacy_ray_amd.vocab.vectors import hash_words

    keys = hash_words(["a", "b", "c"])
    v = Vectors(np.eye(2, dtype="f"), keys, rows=np.array([0, 1, 0]))
    assert v.find_words(["c", "a", "b", "zz"]).tolist() == [0, 0, 1, -1]
    assert v.find_rows(np.zeros(0, np.uint64)).shape == (0,)


# ------------------------------------------------------ configs & modules
def _cfg(static: bool, vectors_dir=None, key_attr_cfg=""):
    return Config.from_str(f"""
[paths]
vectors = null

[nlp]
lang = "en"
pipeline = ["tagger"]

[components]

[components.tagger]
factory = "tagger"

[components.tagger.model]
@architectures = "spacy.Tagger.v2"

[components.tagger.model.tok2vec]
@architectures = "spacy.Tok2Vec.v2"

[components.tagger.model.tok2vec.embed]
@architectures = "spacy.MultiHashEmbed.v2"
width = 32
attrs = ["NORM", "PREFIX", "SUFFIX", "SHAPE"]
rows = [200, 100, 100, 100]
include_static_vectors = {"true" if static else "false"}

[components.tagger.model.tok2vec.encode]
@architectures = "spacy.MaxoutWindowEncoder.v2"
width = 32
depth = 1
window_size = 1
maxout_pieces = 3

[corpora]

[corpora.train]
@readers = "spacy-mi.SyntheticCorpus.v1"
n_docs = 40
words_per_doc = 10
vocab_size = 120
n_tags = 6
seed = 0

[corpora.dev]
@readers = "spacy-mi.SyntheticCorpus.v1"
n_docs = 5
words_per_doc = 10
vocab_size = 120
n_tags = 6
seed = 1

[training]
train_corpus = "corpora.train"
dev_corpus = "corpora.dev"
seed = 0

[training.optimizer]
@optimizers = "Adam.v1"
learn_rate = 0.01

[initialize]
vectors = ${{paths.vectors}}
""", overrides={"paths.vectors": str(vectors_dir)} if vectors_dir else None)


def _lexicon_vectors(tmp_path, n=100, dim=6, key_attr="ORTH"):
    data = np.random.default_rng(1).standard_normal((n, dim)).astype(np.float32)
    Vectors.from_words([f"w{i}" for i in range(n)], data,
                       key_attr=key_attr).to_disk(tmp_path / "vec" / "vocab")
    return tmp_path / "vec", data


# keys of the tagger module above on the parent commit (no static vectors)
PARENT_KEYS = [
    "output.weight", "output.bias",
    "embedded_t2v.embed.tables.0", "embedded_t2v.embed.tables.1",
    "embedded_t2v.embed.tables.2", "embedded_t2v.embed.tables.3",
    "embedded_t2v.embed.mixer.weight", "embedded_t2v.embed.mixer.bias",
    "embedded_t2v.embed.mixer.norm.weight", "embedded_t2v.embed.mixer.norm.bias",
    "embedded_t2v.encode.blocks.0.weight", "embedded_t2v.encode.blocks.0.bias",
    "embedded_t2v.encode.blocks.0.norm.weight",
    "embedded_t2v.encode.blocks.0.norm.bias",
]


def test_pipeline_without_vectors_is_unchanged(tmp_path):
    nlp = init_nlp(_cfg(False), sample_size=8)
    assert nlp.vocab.vectors is None
    module = nlp.get_pipe("tagger").module
    assert list(module.state_dict().keys()) == PARENT_KEYS
    assert module.embedded_t2v.embed.mixer.weight.shape == (96, 128)
    nlp.to_disk(tmp_path / "m")
    assert sorted(p.name for p in (tmp_path / "m" / "vocab").iterdir()) == [
        "strings.json"]
    from spacy_ray_amd.models.batch import TokenBatch

    batch = TokenBatch([Doc(nlp.vocab, ["a", "b"])], "cpu")
    assert batch.vec_rows is None  # nothing extra is shipped


def test_static_vectors_without_a_table_fails_loudly():
    with pytest.raises(ValueError, match=r"\[initialize\] vectors"):
        init_nlp(_cfg(True), sample_size=8)
    with pytest.raises(ValueError, match=r"\[initialize\] vectors"):
        check_static_vectors_config(_cfg(True).interpolate())


def test_debug_config_accepts_the_pair(tmp_path):
    vec_dir, _ = _lexicon_vectors(tmp_path)
    lines = check_static_vectors_config(_cfg(True, vec_dir).interpolate())
    assert lines and "vectors OK" in lines[0]


def test_table_is_data_not_a_parameter(tmp_path):
    vec_dir, data = _lexicon_vectors(tmp_path)
    nlp = init_nlp(_cfg(True, vec_dir), sample_size=8)
    pipe = nlp.get_pipe("tagger")
    module = pipe.module
    keys = list(module.state_dict().keys())
    assert sorted(keys) == sorted(
        PARENT_KEYS + ["embedded_t2v.embed.static_vectors.W"])
    assert module.embedded_t2v.embed.static_vectors.W.shape == (32, 6)
    assert module.embedded_t2v.embed.mixer.weight.shape == (96, 160)
    for t in list(module.state_dict().values()) + list(module.parameters()) + \
            list(module.buffers()):
        assert tuple(t.shape) != data.shape
    n_params = sum(p.numel() for p in module.parameters())
    from spacy_ray_amd.data.thinc_serde import (
        component_to_thinc_nodes, load_thinc_nodes_into_component,
        model_to_thinc_bytes)

    nodes = component_to_thinc_nodes(pipe)
    assert sum(a.size for _, ps in nodes for a in ps.values()) == n_params
    assert ("static_vectors" in [n for n, _ in nodes])
    blob = model_to_thinc_bytes(nodes)
    assert data.tobytes()[:64] not in blob
    # Thinc bytes round-trip, projection included
    torch.manual_seed(5)
    nlp2 = init_nlp(_cfg(True, vec_dir), sample_size=8)
    W2 = nlp2.get_pipe("tagger").module.embedded_t2v.embed.static_vectors.W
    with torch.no_grad():
        W2.add_(1.0)
    assert load_thinc_nodes_into_component(nlp2.get_pipe("tagger"), blob) == len(keys)
    assert torch.equal(W2, module.embedded_t2v.embed.static_vectors.W)


def test_to_disk_from_disk_roundtrips_vectors_exactly(tmp_path):
    vec_dir, data = _lexicon_vectors(tmp_path)
    nlp = init_nlp(_cfg(True, vec_dir), sample_size=8)
    nlp.to_disk(tmp_path / "m")
    nlp2 = init_nlp(_cfg(True, vec_dir), sample_size=8)
    nlp2.vocab.vectors = None
    nlp2.get_pipe("tagger").module = None  # rebuilt from the checkpoint
    nlp2.from_disk(tmp_path / "m")
    a, b = nlp.vocab.vectors, nlp2.vocab.vectors
    assert np.array_equal(a.data, b.data) and a.data.dtype == b.data.dtype
    assert np.array_equal(a.keys, b.keys) and b.keys.dtype == np.uint64
    assert np.array_equal(a.rows, b.rows) and b.rows.dtype == np.int32
    assert (a.name, a.key_attr) == (b.name, b.key_attr)
    docs = [eg.predicted for eg in _examples(nlp)[:5]]
    docs2 = [Doc(nlp2.vocab, d.words) for d in docs]
    nlp.predict_docs(docs)
    nlp2.predict_docs(docs2)
    assert [d.tags for d in docs] == [d.tags for d in docs2]


# --------------------------------------------------------- reference ops
def test_static_vectors_gradcheck_float64():
    from spacy_ray_amd.ops import api as ops

    T, V, nM, nO = 7, 5, 6, 4
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(V, nM, generator=gen, dtype=torch.float64)
    W = torch.randn(nO, nM, generator=gen, dtype=torch.float64, requires_grad=True)
    rows = torch.tensor([0, 3, -1, 3, 4, 1, 2], dtype=torch.int32)
    assert torch.autograd.gradcheck(
        lambda w: ops.static_vectors(w, table, rows), (W,))
    Y = ops.static_vectors(W, table, rows)
    assert torch.equal(Y[2], torch.zeros(nO, dtype=torch.float64))
    assert torch.allclose(Y[1], table[3] @ W.t()) and torch.equal(Y[1], Y[3])
    # no gradient reaches the table
    table.requires_grad_(True)
    ops.static_vectors(W, table, rows).sum().backward()
    assert table.grad is None


# ---------------------------------------------------------------- training
def _examples(nlp):
    from spacy_ray_amd.data.corpus import make_synthetic_docs

    docs = make_synthetic_docs(nlp.vocab, n_docs=40, words_per_doc=10,
                               vocab_size=120, n_tags=6, seed=0)
    return [Example.from_doc(d) for d in docs]


def test_tagger_with_static_vectors_trains(tmp_path):
    vec_dir, data = _lexicon_vectors(tmp_path)
    nlp = init_nlp(_cfg(True, vec_dir), sample_size=8)
    examples = _examples(nlp)
    module = nlp.get_pipe("tagger").module
    W = module.embedded_t2v.embed.static_vectors.W
    opt = torch.optim.Adam(module.parameters(), lr=0.01)
    seen = []
    for step in range(20):
        losses = nlp.update(examples, losses={})
        if step == 1:  # the softmax layer starts at zero: no signal at step 0
            assert W.grad is not None and float(W.grad.abs().sum()) > 0
        opt.step()
        opt.zero_grad()
        seen.append(losses["tagger"])
    assert seen[-1] < 0.8 * seen[0], seen
    assert np.array_equal(nlp.vocab.vectors.data, data)
    assert nlp.vocab.vectors.data.tobytes() == data.tobytes()
    # w100..w119 are out of vocabulary; rows are shared by copy_unannotated
    from spacy_ray_amd.models.batch import TokenBatch

    docs = [eg.predicted for eg in examples]
    batch = TokenBatch(docs, "cpu")
    assert batch.vec_rows.dtype == torch.int32
    assert batch.vec_rows.shape == (batch.n_tokens,)
    words = [w for d in docs for w in d.words]
    want = [int(w[1:]) if int(w[1:]) < 100 else -1 for w in words]
    assert batch.vec_rows.tolist() == want
    assert examples[0].reference.vector_rows is examples[0].predicted.vector_rows
    padded = TokenBatch(docs[:2], "cpu", pad_to=64)
    assert padded.vec_rows.shape == (64,)
    assert (padded.vec_rows[padded.n_real_tokens:] == -1).all()


def test_key_attr_lower_and_orth_differ_for_a_capitalised_word():
    vocab = Vocab("en")
    vocab.vectors = Vectors.from_words(["apple", "Pear"], np.eye(2, dtype="f"))
    doc = Doc(vocab, ["Apple", "apple", "Pear", "pear"])
    assert doc.get_vector_rows("ORTH").tolist() == [-1, 0, 1, -1]
    assert doc.get_vector_rows("LOWER").tolist() == [0, 0, -1, -1]
    assert doc.get_vector_rows("NORM") is not doc.get_vector_rows("LOWER")
    assert doc.get_vector_rows("NORM").tolist() == [0, 0, -1, -1]
    assert doc.get_vector_rows("ORTH") is doc.get_vector_rows("ORTH")


# ------------------------------------------------- Doc / Vocab vector API
def test_doc_vector_similarity_and_vocab_get_vector():
    vocab = Vocab("en")
    assert vocab.vectors is None and not vocab.has_vector("a")
    data = np.random.default_rng(2).standard_normal((3, 4)).astype("f")
    vocab.vectors = Vectors.from_words(["a", "b", "c"], data)
    assert np.array_equal(vocab.get_vector("b"), data[1])
    assert np.array_equal(vocab.get_vector("zzz"), np.zeros(4, "f"))
    d1 = Doc(vocab, ["a", "b", "zzz"])
    assert np.allclose(d1.vector, data[:2].mean(0))
    d2 = Doc(vocab, ["b", "a"])
    assert d1.similarity(d2) == pytest.approx(1.0)
    oov = Doc(vocab, ["x", "y"])
    assert np.array_equal(oov.vector, np.zeros(4, "f"))
    assert d1.similarity(oov) == 0.0
