"""Registered model architectures (the @architectures names spaCy configs
reference — SURVEY.md §5.6; resolution happens when Language builds pipes).

Architecture functions return *model specs* (factory closures) because output
dims (labels) are only known at pipe.initialize() time, mirroring spaCy's
shape-inference-on-sample initialization (`/root/reference/spacy_ray/
worker.py:91` init_nlp contract)."""
from __future__ import annotations

import contextlib
from typing import List, Optional

from spacy_ray_amd.config.registry import registry
from .tok2vec import CharacterEmbed, MaxoutWindowEncoder, MultiHashEmbed, Tok2Vec
from .parser_model import TransitionModel


class ModelSpec:
    """A deferred model constructor: call .build() for the nn.Module."""

    def __init__(self, build, width: Optional[int] = None, kind: str = ""):
        self._build = build
        self.width = width
        self.kind = kind

    def build(self):
        return self._build()


@registry.architectures("spacy.MultiHashEmbed.v2")
def make_multi_hash_embed(
    width: int,
    attrs: List[str] = ("NORM", "PREFIX", "SUFFIX", "SHAPE"),
    rows: List[int] = (5000, 2500, 2500, 2500),
    include_static_vectors: bool = False,
    seed: int = 0,
):
    def build():
        return MultiHashEmbed(
            width, rows=list(rows), attrs=list(attrs), seed=seed,
            include_static_vectors=include_static_vectors,
            vocab=_vocab_for_build() if include_static_vectors else None)

    return ModelSpec(build, width=width, kind="embed")


@registry.architectures("spacy.CharacterEmbed.v2")
def make_character_embed(
    width: int,
    rows: int,
    nM: int,
    nC: int,
    include_static_vectors: bool = False,
    feature: str = "NORM",
):
    if include_static_vectors:
        raise ValueError(
            "spacy.CharacterEmbed.v2: include_static_vectors = true is not "
            "supported yet; use spacy.MultiHashEmbed.v2 for static vectors")
    from spacy_ray_amd.vocab.attrs import ATTR_NAMES

    if feature not in ATTR_NAMES:
        raise ValueError(
            f"spacy.CharacterEmbed.v2: feature must be one of "
            f"{list(ATTR_NAMES)}, got {feature!r}")
    return ModelSpec(
        lambda: CharacterEmbed(width, rows=rows, nM=nM, nC=nC, feature=feature),
        width=width, kind="embed")


# Modules are built inside pipe.initialize / pipe.load_cfg, which know no
# vocab; Language wraps those calls in `building_for(vocab)` so that a
# StaticVectors layer can size its projection from the loaded table.
_BUILD_VOCAB: list = []


@contextlib.contextmanager
def building_for(vocab):
    _BUILD_VOCAB.append(vocab)
    try:
        yield
    finally:
        _BUILD_VOCAB.pop()


def _vocab_for_build():
    vocab = _BUILD_VOCAB[-1] if _BUILD_VOCAB else None
    vectors = getattr(vocab, "vectors", None)
    if vectors is None:
        raise ValueError(
            "include_static_vectors = true but no vectors are loaded: set "
            "[initialize] vectors (or [paths] vectors) to a directory "
            "written by `spacy-mi init vectors`, or set "
            "include_static_vectors = false")
    return vocab


@registry.architectures("spacy.PretrainVectors.v1")
def make_pretrain_vectors(maxout_pieces: int = 3, hidden_size: int = 300,
                          loss: str = "cosine"):
    """`[pretraining.objective]`: predict each masked token's static vector.
    Returns the keyword arguments that select it in
    train.pretrain.pretrain_tok2vec (the head is built there, once the
    tok2vec and the table widths are known)."""
    if loss not in ("cosine", "L2"):
        raise ValueError(
            f"spacy.PretrainVectors.v1: loss must be 'cosine' or 'L2', got {loss!r}")
    return {"objective": "vectors", "loss": loss,
            "hidden_size": int(hidden_size), "maxout_pieces": int(maxout_pieces)}


@registry.architectures("spacy.MaxoutWindowEncoder.v2")
def make_maxout_window_encoder(
    width: int, depth: int = 4, window_size: int = 1, maxout_pieces: int = 3
):
    return ModelSpec(
        lambda: MaxoutWindowEncoder(width, depth=depth, window_size=window_size,
                                    maxout_pieces=maxout_pieces),
        width=width, kind="encode",
    )


@registry.architectures("spacy.Tok2Vec.v2")
def make_tok2vec(embed: ModelSpec, encode: ModelSpec):
    return ModelSpec(lambda: Tok2Vec(embed.build(), encode.build()),
                     width=encode.width, kind="tok2vec")


@registry.architectures("spacy.HashEmbedCNN.v2")
def make_hash_embed_cnn(
    width: int = 96,
    depth: int = 4,
    embed_size: int = 2000,
    window_size: int = 1,
    maxout_pieces: int = 3,
    subword_features: bool = True,
    pretrained_vectors: Optional[str] = None,
):
    rows = [embed_size, embed_size // 2, embed_size // 2, embed_size // 2] if subword_features else [embed_size]
    attrs = ["NORM", "PREFIX", "SUFFIX", "SHAPE"] if subword_features else ["NORM"]

    # spaCy's HashEmbedCNN: any non-null `pretrained_vectors` turns the
    # static-vectors block on; the table itself comes from the vocab
    static = bool(pretrained_vectors)

    def build():
        return Tok2Vec(
            MultiHashEmbed(width, rows=rows, attrs=attrs,
                           include_static_vectors=static,
                           vocab=_vocab_for_build() if static else None),
            MaxoutWindowEncoder(width, depth=depth, window_size=window_size,
                                maxout_pieces=maxout_pieces),
        )

    return ModelSpec(build, width=width, kind="tok2vec")


@registry.architectures("spacy-transformers.TransformerModel.v3")
def make_transformer_model(
    name: str = "roberta-base",
    get_spans=None,
    tokenizer_config: Optional[dict] = None,
    transformer_config: Optional[dict] = None,
    window: int = 128,
    stride: int = 96,
    attn_implementation: str = "sdpa",
    subwords: str = "bpe",
    bpe_vocab_size: int = 8000,
):
    tk = tokenizer_config or {}

    def build():
        from .transformer import TransformerTok2Vec

        return TransformerTok2Vec(name=name, window=window, stride=stride,
                                  transformer_config=transformer_config,
                                  attn_implementation=attn_implementation,
                                  subwords=tk.get("subwords", subwords),
                                  bpe_vocab_size=tk.get("bpe_vocab_size", bpe_vocab_size),
                                  tokenizer_path=tk.get("tokenizer_path"))

    tc = transformer_config or {}
    width = tc.get("hidden_size", 768 if name == "roberta-base" else 64)
    return ModelSpec(build, width=width, kind="tok2vec")


@registry.architectures("spacy.Tok2VecListener.v1")
def make_tok2vec_listener(width: int, upstream: str = "*"):
    return ModelSpec(lambda: None, width=width, kind="listener")


@registry.architectures("spacy.Tagger.v2")
def make_tagger_model(tok2vec: ModelSpec, nO: Optional[int] = None, normalize: bool = False):
    spec = ModelSpec(lambda: None, width=tok2vec.width, kind="tagger")
    # a full tok2vec block (not a listener) => the pipe owns its encoder
    # (spaCy's embedded-tok2vec configuration, e.g. standalone taggers)
    spec.embedded_tok2vec = tok2vec if tok2vec.kind == "tok2vec" else None
    return spec


@registry.architectures("spacy.TransitionBasedParser.v2")
def make_transition_parser_model(
    tok2vec: ModelSpec,
    state_type: str = "parser",
    extra_state_tokens: bool = False,
    hidden_width: int = 64,
    maxout_pieces: int = 2,
    use_upper: bool = True,
    nO: Optional[int] = None,
):
    nF = 13 if state_type == "parser" else 6

    def build():
        return TransitionModel(tok2vec.width, hidden_width=hidden_width, nF=nF)

    spec = ModelSpec(build, width=tok2vec.width, kind=f"transition:{state_type}")
    spec.nF = nF
    spec.hidden_width = hidden_width
    spec.embedded_tok2vec = tok2vec if tok2vec.kind == "tok2vec" else None
    return spec


@registry.architectures("spacy.TextCatCNN.v2")
def make_textcat_cnn_model(tok2vec: ModelSpec, exclusive_classes: bool = True,
                           nO: Optional[int] = None):
    spec = ModelSpec(lambda: None, width=tok2vec.width, kind="textcat")
    spec.embedded_tok2vec = tok2vec if tok2vec.kind == "tok2vec" else None
    return spec


@registry.architectures("spacy.TextCatReduce.v1")
def make_textcat_reduce_model(tok2vec: ModelSpec,
                              exclusive_classes: bool = True,
                              use_reduce_mean: bool = True, **_ignored):
    spec = ModelSpec(lambda: None, width=tok2vec.width, kind="textcat")
    spec.embedded_tok2vec = tok2vec if tok2vec.kind == "tok2vec" else None
    return spec


def _textcat_bow_spec(name: str, ngram_size: int, length: int,
                      no_output_layer: bool = False) -> ModelSpec:
    ngram_size, length = int(ngram_size), int(length)
    if ngram_size < 1:
        raise ValueError(f"{name}: ngram_size must be >= 1, got {ngram_size}")
    if length < 1 or length & (length - 1):
        raise ValueError(
            f"{name}: length must be a power of two (the hashed rows are "
            f"masked with length - 1), got length = {length}")
    # no tok2vec and no width: a bag of hashed token n-grams through Thinc's
    # SparseLinear (ops.sparse_linear); TextcatPipe builds the head
    spec = ModelSpec(lambda: None, width=None, kind="textcat")
    spec.bow = {"ngram_size": ngram_size, "length": length}
    # read by spacy.TextCatEnsemble.v2 alone; kept out of spec.bow, which a
    # BOW pipe writes into its cfg
    spec.no_output_layer = bool(no_output_layer)
    return spec


@registry.architectures("spacy.TextCatBOW.v2")
def make_textcat_bow_v2(exclusive_classes: bool = True, ngram_size: int = 1,
                        no_output_layer: bool = False, nO: Optional[int] = None):
    """spaCy's efficiency-mode text classifier.  `no_output_layer` changes
    nothing here: the softmax / sigmoid lives in the loss and in prediction
    (spacy.TextCatEnsemble.v2 honours it for its BOW branch)."""
    return _textcat_bow_spec("spacy.TextCatBOW.v2", ngram_size, 262144, no_output_layer)


@registry.architectures("spacy.TextCatBOW.v3")
def make_textcat_bow_v3(exclusive_classes: bool = True, ngram_size: int = 1,
                        no_output_layer: bool = False, length: int = 262144,
                        nO: Optional[int] = None):
    return _textcat_bow_spec("spacy.TextCatBOW.v3", ngram_size, length, no_output_layer)


@registry.architectures("spacy.TextCatEnsemble.v2")
def make_textcat_ensemble(tok2vec: ModelSpec, linear_model: ModelSpec,
                          nO: Optional[int] = None):
    """spaCy's accuracy-mode text classifier: a BOW branch (ops.sparse_linear,
    through softmax / sigmoid unless its `no_output_layer` is set) next to
    the tok2vec pooled by attention (ops.attention_pool) with a Maxout +
    LayerNorm residual, concatenated into one output layer.  TextcatPipe
    builds the head (TextcatEnsembleHead)."""
    bow = getattr(linear_model, "bow", None)
    if not isinstance(linear_model, ModelSpec) or bow is None:
        raise ValueError(
            "spacy.TextCatEnsemble.v2: linear_model must be a spacy.TextCatBOW.v2 "
            f"or .v3 block, got {linear_model!r}")
    spec = ModelSpec(lambda: None, width=tok2vec.width, kind="textcat")
    spec.embedded_tok2vec = tok2vec if tok2vec.kind == "tok2vec" else None
    spec.attention = {"keys": False, "bow": dict(bow),
                      "no_output_layer": bool(linear_model.no_output_layer)}
    return spec


@registry.architectures("spacy.TextCatParametricAttention.v1")
def make_textcat_parametric_attention(tok2vec: ModelSpec,
                                      exclusive_classes: bool = True,
                                      nO: Optional[int] = None):
    """The ensemble's attention branch alone, with Thinc's Gelu(width ->
    width) key transform in front of the attention, and an output layer."""
    spec = ModelSpec(lambda: None, width=tok2vec.width, kind="textcat")
    spec.embedded_tok2vec = tok2vec if tok2vec.kind == "tok2vec" else None
    spec.attention = {"keys": True, "bow": None, "no_output_layer": False}
    return spec


@registry.layers("spacy.mean_max_reducer.v1")
def make_mean_max_reducer(hidden_size: int = 128):
    """spaCy's span reducer: last | first | mean | max over the span's
    tokens, then Maxout(nO=hidden_size, nP=3, normalize=True).  Returns the
    settings; SpancatPipe builds the head once the labels are known."""
    if int(hidden_size) < 1:
        raise ValueError("spacy.mean_max_reducer.v1: hidden_size must be >= 1")
    return {"reducer": "mean_max", "hidden_size": int(hidden_size)}


@registry.layers("spacy.LinearLogistic.v1")
def make_linear_logistic(nO: Optional[int] = None, nI: Optional[int] = None):
    """spaCy's span scorer: a linear layer whose logits go through a
    sigmoid (in the loss and at prediction time)."""
    return {"scorer": "linear_logistic"}


@registry.architectures("spacy.SpanCategorizer.v1")
def make_spancat_model(tok2vec: ModelSpec, reducer: Optional[dict] = None,
                       scorer: Optional[dict] = None, **_ignored):
    """Without a `reducer` block: mean pooling and one linear layer
    (SpancatHead).  With `spacy.mean_max_reducer.v1`: spaCy's model, the
    span-pool kernels + Maxout + linear-logistic scorer."""
    for block, key in ((reducer, "reducer"), (scorer, "scorer")):
        if block is not None and not (isinstance(block, dict) and key in block):
            raise ValueError(
                f"spacy.SpanCategorizer.v1: unsupported {key} block {block!r}")
    if scorer is not None and reducer is None:
        raise ValueError(
            "spacy.SpanCategorizer.v1: a scorer block needs a reducer block")
    spec = ModelSpec(lambda: None, width=tok2vec.width, kind="spancat")
    spec.embedded_tok2vec = tok2vec if tok2vec.kind == "tok2vec" else None
    spec.hidden_size = reducer["hidden_size"] if reducer else None
    return spec
