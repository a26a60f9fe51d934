"""CLI + launcher: end-to-end 2-worker gloo run, checkpoints, resume,
fault supervision.  These spawn subprocesses (slow-ish but the real path)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
CFG = REPO / "examples" / "configs" / "en_tagger_cpu.cfg"


def _run_cli(args, env_extra=None, timeout=420):
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    env.update(env_extra or {})
    return subprocess.run(
        [sys.executable, "-m", "spacy_ray_amd.cli.main", "ray", "train", *args],
        cwd=str(REPO), env=env, capture_output=True, text=True, timeout=timeout,
    )


def test_cli_two_workers_checkpoint_and_metrics(tmp_path):
    out = tmp_path / "out"
    r = _run_cli([str(CFG), "--n-workers", "2", "--output", str(out),
                  "--training.max_steps", "8", "--training.eval_frequency", "4"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert (out / "model-last" / "config.cfg").exists()
    assert (out / "model-last" / "tagger" / "model.safetensors").exists()
    assert (out / "model-last" / "optim.rank0.pt").exists()
    assert (out / "model-last" / "optim.rank1.pt").exists()
    lines = (out / "metrics.jsonl").read_text().strip().splitlines()
    rec = json.loads(lines[-1])
    assert rec["step"] >= 4 and "wps" in rec
    # model-best written at the eval checkpoint
    assert (out / "model-best" / "meta.json").exists()


def test_cli_single_worker_inprocess(tmp_path):
    out = tmp_path / "out1"
    r = _run_cli([str(CFG), "--output", str(out), "--training.max_steps", "4",
                  "--training.eval_frequency", "2"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert (out / "model-last" / "config.cfg").exists()


def test_launcher_aborts_all_on_rank_failure(tmp_path):
    out = tmp_path / "out2"
    r = _run_cli([str(CFG), "--n-workers", "2", "--output", str(out),
                  "--training.max_steps", "50", "--training.eval_frequency", "50"],
                 env_extra={"SRX_FAULT_INJECT": "1:2"})
    assert r.returncode != 0  # supervisor propagates the failure


def test_finite_epochs_uneven_shards_no_hang(tmp_path):
    """2 workers, odd corpus size, finite epochs: per-rank batch counts can
    differ — the per-step agreement collective must end training cleanly on
    every rank (regression test for the finite-epoch hang)."""
    out = tmp_path / "outfe"
    r = _run_cli([str(CFG), "--n-workers", "2", "--output", str(out),
                  "--corpora.train.n_docs", "401",
                  "--training.max_epochs", "2",
                  "--training.max_steps", "0",
                  "--training.eval_frequency", "5"], timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (out / "model-last" / "config.cfg").exists()


def test_resume_continues_from_checkpoint(tmp_path):
    out = tmp_path / "outr"
    r = _run_cli([str(CFG), "--n-workers", "2", "--output", str(out),
                  "--training.max_steps", "6", "--training.eval_frequency", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    before = (out / "model-last" / "tagger" / "model.safetensors").read_bytes()
    r = _run_cli([str(CFG), "--n-workers", "2", "--output", str(out), "--resume",
                  "--training.max_steps", "3", "--training.eval_frequency", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    after = (out / "model-last" / "tagger" / "model.safetensors").read_bytes()
    assert before != after  # training continued and re-saved


def test_cli_evaluate(tmp_path):
    out = tmp_path / "oute"
    r = _run_cli([str(CFG), "--output", str(out), "--training.max_steps", "6",
                  "--training.eval_frequency", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    r = subprocess.run(
        [sys.executable, "-m", "spacy_ray_amd.cli.main", "ray", "evaluate",
         str(out / "model-last")],
        cwd=str(REPO), env=env, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    scores = json.loads(r.stdout)
    assert "tag_acc" in scores and "score" in scores


def test_overrides_reach_workers(tmp_path):
    out = tmp_path / "out3"
    r = _run_cli([str(CFG), "--n-workers", "2", "--output", str(out),
                  "--training.max_steps", "3", "--training.eval_frequency", "2",
                  "--components.tok2vec.model.width", "64",
                  "--components.tagger.model.tok2vec.width", "64"])
    assert r.returncode == 0, r.stderr[-3000:]
    cfg_text = (out / "model-last" / "config.cfg").read_text()
    assert '"width": 64' in cfg_text or "width = 64" in cfg_text


def test_multinode_emulation_two_launchers(tmp_path):
    """Two launcher invocations on localhost emulate a 2-node run: each node
    contributes one worker (--nnodes 2 --node-rank r --address host:port);
    global ranks must be unique and training completes on both."""
    import socket
    import threading

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = tmp_path / "outmn"
    results = {}

    def node(rank):
        results[rank] = _run_cli(
            [str(CFG), "--n-workers", "1", "--output", str(out),
             "--address", f"127.0.0.1:{port}", "--nnodes", "2",
             "--node-rank", str(rank),
             "--training.max_steps", "6", "--training.eval_frequency", "3"])

    threads = [threading.Thread(target=node, args=(r,)) for r in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=420)
    for r in (0, 1):
        assert results[r].returncode == 0, (r, results[r].stderr[-3000:])
    assert (out / "model-last" / "config.cfg").exists()
    assert (out / "model-last" / "optim.rank0.pt").exists()
    assert (out / "model-last" / "optim.rank1.pt").exists()


def test_cli_evaluate_saved_model(tmp_path):
    """`spacy-mi ray evaluate <model-dir>` loads a checkpoint and prints a
    scores JSON including the weighted composite."""
    out = tmp_path / "outev"
    r = _run_cli([str(CFG), "--output", str(out), "--training.max_steps", "4",
                  "--training.eval_frequency", "2"])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    r2 = subprocess.run(
        [sys.executable, "-m", "spacy_ray_amd.cli.main", "ray", "evaluate",
         str(out / "model-last")],
        cwd=str(REPO), env=env, capture_output=True, text=True, timeout=300,
    )
    assert r2.returncode == 0, r2.stderr[-3000:]
    scores = json.loads(r2.stdout)
    assert "score" in scores and "tag_acc" in scores


def test_code_injection_custom_reader(tmp_path):
    """--code imports user code on every worker before config resolution:
    a custom @readers function defined in the user file must resolve
    (the reference's import_code contract, train_cli.py --code)."""
    code = tmp_path / "user_code.py"
    code.write_text("""
from spacy_ray_amd.config.registry import registry
from spacy_ray_amd.data.corpus import create_synthetic_corpus

@registry.readers("user.TinyCorpus.v1")
def tiny_corpus(seed: int = 0):
    return create_synthetic_corpus(n_docs=40, words_per_doc=8, vocab_size=50,
                                   n_tags=5, seed=seed)
""")
    cfg_text = CFG.read_text().replace(
        '@readers = "spacy-mi.SyntheticCorpus.v1"', "@@MARK@@", 1)
    # replace the train corpus block with the custom reader (strip its kwargs)
    lines, out_lines, in_train = cfg_text.splitlines(), [], False
    for l in lines:
        if l == "@@MARK@@":
            in_train = True
            out_lines.append('@readers = "user.TinyCorpus.v1"')
            continue
        if in_train:
            if l.startswith("[") or not l.strip():
                in_train = False
                out_lines.append(l)
            continue  # drop synthetic kwargs
        out_lines.append(l)
    cfg_path = tmp_path / "cfg.cfg"
    cfg_path.write_text("\n".join(out_lines))
    out = tmp_path / "out"
    r = _run_cli([str(cfg_path), "--code", str(code), "--output", str(out),
                  "--training.max_steps", "2", "--training.eval_frequency", "2"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert (out / "model-last" / "config.cfg").exists()


@pytest.mark.parametrize("world", [2, 4])
def test_bench_multirank_gloo(tmp_path, world):
    """The driver's SCALE run launches bench.py under torch.distributed.run
    with N ranks; exercise that exact path on CPU/gloo and check rank 0
    prints one valid JSON line.  world=4 regresses the warmup-count
    deadlock: per-rank len(batches) differ, so the warmup step count must
    be the global max or ranks issue mismatched collective sequences."""
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
         "--master-port", str(29530 + world), str(REPO / "bench.py"),
         "--gpus", str(world), "--steps", "2", "--warmup", "1",
         "--batch-words", "1500"],
        cwd=str(REPO), env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    json_lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(json_lines) == 1, r.stdout[-1500:]
    rec = json.loads(json_lines[0])
    assert rec["steps"] == 2 and rec["scaling"] == "weak"
    assert rec["config"]["parallelism"] == f"dp{world}"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes each timed step's losses and the parameter norms
    after the last step as float64 .npy; the same arguments give the same
    inputs, so on the deterministic CPU path two runs dump identical arrays.
    --steps sets the number of timed steps: one loss per step."""
    import numpy as np

    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    dumps = []
    for tag in ("a", "b"):
        out = tmp_path / tag
        r = subprocess.run(
            [sys.executable, str(REPO / "bench.py"), "--gpus", "1",
             "--steps", "3", "--warmup", "1", "--batch-words", "400",
             "--dump-outputs", str(out)],
            cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600,
        )
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
        json_lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(json_lines) == 1, r.stdout[-1500:]
        rec = json.loads(json_lines[0])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        files = sorted(out.glob("*.npy"))
        assert {f.name for f in files} == {"loss_tagger.npy", "loss_parser.npy",
                                           "loss_ner.npy", "param_norms.npy"}
        assert sum(f.stat().st_size for f in files) <= 64 << 20
        arrays = {f.name: np.load(f) for f in files}
        for name, a in arrays.items():
            assert a.dtype == np.float64 and np.isfinite(a).all(), (name, a.dtype)
            if name.startswith("loss_"):
                assert a.shape == (3,) and (a > 0).all(), (name, a)
        assert arrays["param_norms.npy"].size > 10
        dumps.append(arrays)
    for name in dumps[0]:
        np.testing.assert_array_equal(dumps[0][name], dumps[1][name], err_msg=name)


def test_bench_full_runs_sweep_then_headline(monkeypatch, capfd):
    """--full: one JSON line per sweep size from child processes, then the
    headline run's line last.  The sweep sizes are shrunk to CPU scale."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_under_test", REPO / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "FULL_BATCH_WORDS", (200, 300, 400))
    monkeypatch.setenv("PYTHONPATH", str(REPO))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2",
                                      "--warmup", "1", "--batch-words", "600",
                                      "--full"])
    bench.main()
    out = capfd.readouterr().out
    recs = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert len(recs) == 4, out[-1500:]
    sizes = [r["config"]["global_batch"] for r in recs]
    for got, want in zip(sizes, (200, 300, 400, 600)):
        assert want <= got < want + 100, sizes
    assert all(r["steps"] == 2 and r["value"] > 0 and r["ms_per_step"] > 0
               for r in recs)


def test_resume_does_not_overwrite_better_model_best(tmp_path):
    """model-best's meta.json carries the composite best_score; a resumed
    run seeded with it must not overwrite model-best unless it actually
    beats it."""
    out = tmp_path / "outrb"
    r = _run_cli([str(CFG), "--output", str(out), "--training.max_steps", "6",
                  "--training.eval_frequency", "3"])
    assert r.returncode == 0, r.stderr[-3000:]
    meta_path = out / "model-best" / "meta.json"
    meta = json.loads(meta_path.read_text())
    assert "best_score" in meta
    # pretend the previous run reached a near-perfect score
    meta["best_score"] = 0.999
    meta["sentinel"] = "previous-best"
    meta_path.write_text(json.dumps(meta))
    r2 = _run_cli([str(CFG), "--output", str(out), "--resume",
                   "--training.max_steps", "6",
                   "--training.eval_frequency", "3"])
    assert r2.returncode == 0, r2.stderr[-3000:]
    meta2 = json.loads(meta_path.read_text())
    assert meta2.get("sentinel") == "previous-best"  # not overwritten


def test_use_averages_checkpoints_hold_averaged_params(tmp_path):
    """With use_averages, saved checkpoints must contain the running
    parameter AVERAGE (what eval scored), not the live trained params —
    the spaCy `nlp.use_params(optimizer.averages)` save contract."""
    import torch

    import spacy_ray_amd
    import spacy_ray_amd.train.worker as wm
    from spacy_ray_amd.config.config import Config
    from spacy_ray_amd.train.worker import distributed_train

    captured = {}
    orig_engine = wm.ZeRO1Engine

    class Capture(orig_engine):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            captured["engine"] = self

    wm.ZeRO1Engine = Capture
    out = tmp_path / "outavg"
    try:
        distributed_train(
            Config.from_disk(CFG, overrides={
                "training.max_steps": 6, "training.eval_frequency": 3,
                "training.optimizer.use_averages": True}),
            output_path=out, use_gpu=-1)
    finally:
        wm.ZeRO1Engine = orig_engine
    engine = captured["engine"]
    nlp = engine.nlp
    nlp2 = spacy_ray_amd.load(out / "model-last")
    live = [p.detach().clone() for p in nlp.torch_module().parameters()]
    with engine.averaged_params():
        avg = [p.detach().clone() for p in nlp.torch_module().parameters()]
    saved = list(nlp2.torch_module().parameters())
    # averages differ from live after a few steps ...
    assert any(not torch.allclose(l, a) for l, a in zip(live, avg))
    # ... and the checkpoint matches the AVERAGED params
    for a, s in zip(avg, saved):
        assert torch.allclose(a.float(), s.float(), atol=1e-6), "saved != averaged"


def _run_sub(args, timeout=240):
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    return subprocess.run(
        [sys.executable, "-m", "spacy_ray_amd.cli.main", *args],
        cwd=str(REPO), env=env, capture_output=True, text=True, timeout=timeout,
    )


def test_debug_config_ok_and_fails_on_bad():
    r = _run_sub(["debug", "config", str(CFG)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "config OK" in r.stdout
    # a broken override must exit nonzero
    r2 = _run_sub(["debug", "config", str(CFG), "--training.dropout", "5.0"])
    assert r2.returncode != 0


def test_debug_data_reports_counts(tmp_path):
    r = _run_sub(["debug", "data", str(CFG), "--limit", "50"])
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert "train:" in r.stdout and "dev:" in r.stdout
    assert "tokens" in r.stdout


def test_init_config_generates_trainable_config(tmp_path):
    """init config -> debug config passes -> a short training run works when
    pointed at a converted DocBin corpus."""
    cfg_path = tmp_path / "gen.cfg"
    r = _run_sub(["init", "config", str(cfg_path),
                  "--pipeline", "tagger,ner", "--arch", "cnn", "--width", "32"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert cfg_path.exists()
    r2 = _run_sub(["debug", "config", str(cfg_path)])
    assert r2.returncode == 0, (r2.stdout[-500:], r2.stderr[-2000:])

    # make a tiny corpus and train 2 steps through the generated config
    from spacy_ray_amd.data.docbin import DocBin
    from spacy_ray_amd.vocab.doc import Doc, Vocab

    v = Vocab()
    docs = [Doc(v, [f"w{i}", "x", "y"], tags=["A", "B", "A"],
                ents=["U-ORG", "O", "O"]) for i in range(40)]
    bin_path = tmp_path / "train.spacy"
    DocBin(docs).to_disk(bin_path)
    r3 = _run_cli([str(cfg_path), "--output", str(tmp_path / "m"),
                   "--paths.train", str(bin_path), "--paths.dev", str(bin_path),
                   "--training.max_steps", "2", "--training.eval_frequency", "2",
                   "--training.batcher.size", "200"])
    assert r3.returncode == 0, r3.stderr[-3000:]
    assert (tmp_path / "m" / "model-last" / "config.cfg").exists()


def test_init_config_trf_stdout():
    r = _run_sub(["init", "config", "-", "--arch", "trf", "--pipeline", "tagger"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "spacy-transformers.TransformerModel.v3" in r.stdout
    assert "ner" not in r.stdout.split("[nlp]")[1].split("[components]")[0]


def test_debug_data_with_path_overrides(tmp_path):
    """debug data accepts --paths.* overrides like train does (the
    quickstart flow: generated config + converted DocBin paths)."""
    cfg_path = tmp_path / "gen.cfg"
    assert _run_sub(["init", "config", str(cfg_path),
                     "--pipeline", "tagger"]).returncode == 0
    from spacy_ray_amd.data.docbin import DocBin
    from spacy_ray_amd.vocab.doc import Doc, Vocab

    v = Vocab()
    docs = [Doc(v, ["a", "b"], tags=["X", "Y"]) for _ in range(10)]
    bin_path = tmp_path / "d.spacy"
    DocBin(docs).to_disk(bin_path)
    r = _run_sub(["debug", "data", str(cfg_path),
                  "--paths.train", str(bin_path), "--paths.dev", str(bin_path)])
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-1500:])
    assert "10 docs" in r.stdout


def test_cli_package_wraps_trained_model(tmp_path):
    """spacy-mi package: trained dir -> pip-shaped package whose load()
    restores a working pipeline."""
    import subprocess
    import sys

    out = tmp_path / "model"
    r = _run_cli([str(CFG), "--output", str(out), "--training.max_steps", "2",
                  "--training.eval_frequency", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    pkg_out = tmp_path / "pkg"
    r2 = subprocess.run(
        [sys.executable, "-m", "spacy_ray_amd.cli.main", "package",
         str(out / "model-last"), str(pkg_out), "--name", "demo",
         "--version", "1.2.3"],
        cwd=str(REPO), capture_output=True, text=True, timeout=300,
    )
    assert r2.returncode == 0, r2.stderr[-2000:]
    root = pkg_out / "en_demo-1.2.3"
    assert (root / "setup.py").exists()
    assert (root / "en_demo" / "__init__.py").exists()
    assert (root / "en_demo" / "en_demo-1.2.3" / "meta.json").exists()
    # import the generated module (no pip: path injection) and load()
    import importlib.util

    spec = importlib.util.spec_from_file_location(
        "en_demo", root / "en_demo" / "__init__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    nlp = mod.load()
    doc = nlp("Don't panic!")
    assert doc.tags is not None and len(doc.tags) == len(doc)


def test_assemble_and_apply_cli(tmp_path):
    """`assemble` builds+saves an untrained pipeline; `apply` annotates a
    DocBin or a text file with a saved pipeline (spaCy CLI roles)."""
    import subprocess
    import sys

    from spacy_ray_amd.data.docbin import DocBin
    from spacy_ray_amd.vocab.doc import Doc, Vocab

    asm = tmp_path / "asm"
    r = subprocess.run(
        [sys.executable, "-m", "spacy_ray_amd.cli.main", "assemble",
         "examples/configs/en_tagger_cpu.cfg", str(asm)],
        capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr[-800:]
    assert (asm / "config.cfg").exists() and (asm / "tagger").exists()
    # apply over a DocBin
    v = Vocab()
    din = tmp_path / "in.spacy"
    DocBin([Doc(v, ["hello", "world"]), Doc(v, ["again"])]).to_disk(din)
    dout = tmp_path / "out.spacy"
    r = subprocess.run(
        [sys.executable, "-m", "spacy_ray_amd.cli.main", "apply",
         str(asm), str(din), str(dout)],
        capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr[-800:]
    docs = list(DocBin.from_disk(dout, v).get_docs(v))
    assert len(docs) == 2
    assert docs[0].tags and len(docs[0].tags) == 2


def test_init_fill_config_cli(tmp_path):
    """`init fill-config` materializes [training] schema defaults while
    preserving existing values."""
    import subprocess
    import sys

    base = tmp_path / "partial.cfg"
    base.write_text('[nlp]\nlang = "en"\npipeline = ["tok2vec","tagger"]\n\n'
                    '[training]\nmax_steps = 500\n')
    out = tmp_path / "full.cfg"
    r = subprocess.run(
        [sys.executable, "-m", "spacy_ray_amd.cli.main", "init",
         "fill-config", str(base), str(out)],
        capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr[-800:]
    from spacy_ray_amd.config.config import Config

    cfg = Config.from_disk(out)
    t = cfg["training"]
    assert t["max_steps"] == 500          # preserved
    assert t["dropout"] == 0.1            # defaulted
    assert t["eval_frequency"] == 200     # defaulted
