"""CPU tests of the host logic around the kernels: shard format, rank slice + shift against the
fixtures the reference produced, and the world_size-2 batch-sharded path over gloo."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import golden_inputs as gi
from oracle import oracle as orc

G = gi.GOLDEN_DIR
REPO = Path(__file__).resolve().parent.parent


def test_shard_roundtrip_and_bad_header(tmp_path):
    from mixture_of_tokenizers_amd import loader
    toks = np.random.RandomState(0).randint(0, 50257, size=5000)
    f = tmp_path / "fineweb_train_000001.bin"
    loader.write_data_shard(f, toks)
    got = loader.read_shard(f)
    assert got.dtype == torch.uint16 and got.numel() == 5000
    np.testing.assert_array_equal(got.numpy().astype(np.int64), toks)
    raw = bytearray(f.read_bytes())
    assert int.from_bytes(raw[0:4], "little") == 20240520 and int.from_bytes(raw[8:12], "little") == 5000
    bad = tmp_path / "fineweb_train_000000.bin"
    raw[0] = 0
    bad.write_bytes(bytes(raw))
    with pytest.raises(AssertionError, match="magic"):
        loader.read_shard(bad)
    # the stream skips the bad shard (train_gpt.py:641-648) and holds int32
    st = loader.ShardStream([bad, f])
    assert st.buffer.dtype == torch.int32 and st.buffer.numel() == 5000 and st.remaining() == 5000


def test_shard_stream_crosses_shards_like_the_reference(tmp_path):
    """ShardStream against the reference's cursor arithmetic written out on plain arrays (train_gpt.py:798-805): a batch is taken
    at `pos`; when `pos + window + 1 >= len(data)` the next shard is appended and `pos` goes back to 0 (the reference's rewind
    into tokens already served -- reproduced, not fixed); uint16 shards and an int32 shard under bytes/ mix; a shard with a bad
    header is skipped; running out of shards ends in RuntimeError (PEP 479 in the reference's generator)."""
    from mixture_of_tokenizers_amd import loader
    rs = np.random.RandomState(5)
    (tmp_path / "bytes").mkdir()
    shards, paths = [], []
    for i, (n, wide) in enumerate(((700, False), (333, False), (1200, True), (90, False))):
        toks = rs.randint(0, 70000 if wide else 50257, size=n)
        f = (tmp_path / "bytes" if wide else tmp_path) / f"train_{i:06d}.bin"
        loader.write_data_shard(f, toks, dtype=np.int32 if wide else np.uint16)
        shards.append(toks); paths.append(f)
    bad = tmp_path / "train_bad.bin"
    bad.write_bytes(b"\x00" * 2048)
    order = [paths[0], bad, paths[1], paths[2], paths[3]]
    window = 4 * 33
    st = loader.ShardStream(order)
    data, pos, nxt, served = shards[0].copy(), 0, 1, 0
    with pytest.raises(RuntimeError, match="StopIteration"):
        while True:
            if pos + window + 1 >= len(data):           # the reference's condition and reset, on numpy arrays
                if nxt >= len(shards):
                    st.advance(window)                  # must raise here too
                    raise AssertionError("ShardStream found a shard the reference stream does not have")
                data, pos, nxt = np.concatenate([data, shards[nxt]]), 0, nxt + 1
            start = st.advance(window)
            assert start == pos and st.remaining() == len(data) - pos - window
            np.testing.assert_array_equal(st.buffer[start:start + window].numpy(), data[pos:pos + window])
            for rank in range(2):
                got = loader.rank_slice(st.buffer, start, 4, 32, rank, 2)
                np.testing.assert_array_equal(got.numpy(), data[pos + rank * window // 2:][:window // 2].reshape(-1, 33))
            pos += window
            served += 1
    assert served > 12 and nxt == len(shards)


def test_batch_file_roundtrip(tmp_path):
    """save_file / load_file (data_creation.py:405-459): the packed (B, T, 1 + 4*bpt) batch as an int32 shard, and the
    reference's verify_data check (462-470) on it."""
    from mixture_of_tokenizers_amd import loader
    B, T, bpt = 2, 5, 4
    batch = torch.randint(0, 458, (B, T, 1 + 4 * bpt), dtype=torch.int64)
    loader.save_file(str(tmp_path / "b.bin"), batch)
    back = loader.load_file(str(tmp_path / "b.bin"))
    assert back.dtype == torch.int32 and back.numel() == batch.numel()
    assert torch.equal(back.view(B, T, 1 + 4 * bpt).to(torch.int64), batch)


def test_rank_slice_and_shift_match_reference_fixture():
    from mixture_of_tokenizers_amd import loader
    z = np.load(G / "loader.npz")
    data = torch.from_numpy(z["data"])
    pos, batch, seq = int(z["pos"]), int(z["batch"]), int(z["seq"])
    for world in (1, 2, 4):
        rows = []
        for rank in range(world):
            toks = loader.rank_slice(data, pos, batch, seq, rank, world)
            assert toks.shape == (batch // world, seq + 1)
            np.testing.assert_array_equal(toks[:, :-1].numpy(), z[f"w{world}r{rank}/toks_in"])
            np.testing.assert_array_equal(toks[:, 1:].numpy(), z[f"w{world}r{rank}/targets"])
            rows.append(toks)
        # the shards tile the global batch exactly: no overlap, no gap
        assert torch.equal(torch.cat(rows), loader.rank_slice(data, pos, batch, seq, 0, 1))
    with pytest.raises(AssertionError):
        loader.rank_slice(data, pos, batch, seq, 0, 3)      # train_gpt.py:795


def test_digit_table_matches_the_reference():
    """make_digit_table == GenerateEquations.tokens_to_digits applied to every token id (mathblations/data.py:92-109)."""
    from mixture_of_tokenizers_amd import data_creation as dc
    z = np.load(G / "mathblations_c1.npz")
    np.testing.assert_array_equal(dc.make_digit_table(3).numpy(), z["digit_table"])
    t2 = dc.make_digit_table(2).numpy()              # another width against the oracle's restatement
    np.testing.assert_array_equal(t2, orc.tokens_to_digits(np.arange(103), 2).reshape(103, 2))
    with pytest.raises(AssertionError):
        dc.make_digit_table(0)


def test_create_data_dispatch_keys():
    from mixture_of_tokenizers_amd import loader
    from mixture_of_tokenizers_amd.modules import ByteHyperparameters
    ok = ByteHyperparameters(byte_mixin_method="concat", pull_in=True, byte_mixout_method="noop", pull_out=False)
    loader.make_create_data_from_toks(ok, None, None)
    with pytest.raises(KeyError):   # (True, False, True, False) is not a key of the reference's table (train_gpt.py:766-776)
        loader.make_create_data_from_toks(
            ByteHyperparameters(byte_mixin_method="concat", pull_in=False, byte_mixout_method="copy", pull_out=False), None, None)


def test_module_names_and_state_dict_keys():
    """Optimizer groups and checkpoints are built from these names (train_gpt.py:1124-1157)."""
    from mixture_of_tokenizers_amd import modules as M
    bp = M.ByteHyperparameters(byte_mixin_method="concat", bytes_per_token=16)
    dims = M.ModelDims(model_dim=1024, byte_dim=48, token_dim=256)

    class Host(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.embed = M.FlexibleEmbedding(dims, 50257, bp)
            self.byte_mixin = M.ByteMixin(dims, 1024, bp)

    h = Host()
    assert list(h.state_dict()) == ["embed.embed_tokens.weight", "embed.embed_bytes.weight", "byte_mixin.mixin.mixin.weight"]
    assert h.byte_mixin.mixin.mixin.weight.shape == (1024, 256 + 16 * 48)
    assert isinstance(h.embed.embed_tokens, torch.nn.Embedding) and isinstance(h.byte_mixin.mixin.attention, torch.nn.Identity)
    assert [n for n, _ in h.named_parameters() if "embed" in n] == ["embed.embed_tokens.weight", "embed.embed_bytes.weight"]
    w = h.byte_mixin.mixin.mixin.weight
    bound = (3 ** 0.5) * 0.5 * w.shape[1] ** -0.5
    assert float(w.detach().abs().max()) <= bound                      # CastedLinear init, train_gpt.py:179-183
    noop = M.ByteHyperparameters(byte_mixin_method="noop")
    e = M.FlexibleEmbedding(dims, 100, noop)
    assert e.embed_tokens.weight.shape == (100, 1024) and isinstance(e.embed_bytes, torch.nn.Identity)   # train_gpt.py:330-331
    with pytest.raises(RuntimeError, match="Invalid byte mixin method"):
        M.ByteMixin(dims, 8, M.ByteHyperparameters(byte_mixin_method="bogus"))
    cfg = M.GPTConfig(vocab_size=1003, n_embd_tok=256, n_embd_digit=256, length_factor=3, digit_mixin_method="concat")
    fe = M.DigitFrontEnd(cfg)
    assert list(fe.state_dict()) == ["wte.weight", "dte.weight", "digit_mixin.fc.weight", "digit_mixin.fc.bias"]
    assert fe.digit_mixin.fc.weight.shape == (256, 1024)
    with pytest.raises(AssertionError, match="Digits must be provided"):
        fe(torch.zeros(1, 4, dtype=torch.long), None)


# ---------------------------------------------------------------------------------------------
# world_size 2 over gloo: every rank runs the front-end's integer path (the oracle stands in for the
# GPU kernels on this CPU-only host) on its shard; the only collective is the counter all-reduce.
# ---------------------------------------------------------------------------------------------
def _worker(rank, world, port, tmp):
    sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mixture_of_tokenizers_amd import loader
    z = np.load(G / "loader.npz")
    data = torch.from_numpy(z["data"])
    pos, batch, seq = int(z["pos"]), int(z["batch"]), int(z["seq"])
    toks = loader.rank_slice(data, pos, batch, seq, rank, world)
    bpt = 16
    tab = gi.synth_ttb(3001, 512, bpt, "left").astype(np.float32)
    padded = orc.tokens_to_bytes(toks.numpy(), tab)
    pulled = orc.pull_from_left(padded, bpt, gi.PAD, gi.EOT)
    st = orc.byte_stats(padded, pulled, gi.PAD)
    counters = torch.tensor([toks.numel(), int(st[0]), int(st[1]), int(st[2])], dtype=torch.int64)
    dist.all_reduce(counters, op=dist.ReduceOp.SUM)          # what bench.py does over RCCL
    gathered = [torch.empty_like(torch.from_numpy(pulled)) for _ in range(world)]
    dist.all_gather(gathered, torch.from_numpy(pulled))
    if rank == 0:
        torch.save(dict(counters=counters, pulled=torch.cat(gathered)), tmp)
    dist.barrier()
    dist.destroy_process_group()


def test_world_size_2_gloo(tmp_path):
    out = tmp_path / "w2.pt"
    port = 29500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(out)), nprocs=2, join=True)
    res = torch.load(out)
    from mixture_of_tokenizers_amd import loader
    z = np.load(G / "loader.npz")
    data = torch.from_numpy(z["data"])
    pos, batch, seq = int(z["pos"]), int(z["batch"]), int(z["seq"])
    toks = loader.rank_slice(data, pos, batch, seq, 0, 1).numpy()
    tab = gi.synth_ttb(3001, 512, 16, "left").astype(np.float32)
    padded = orc.tokens_to_bytes(toks, tab)
    pulled = orc.pull_from_left(padded, 16, gi.PAD, gi.EOT)
    np.testing.assert_array_equal(res["pulled"].numpy(), pulled)         # sharded == unsharded, bit for bit
    st = orc.byte_stats(padded, pulled, gi.PAD)
    assert res["counters"].tolist() == [toks.size, int(st[0]), int(st[1]), int(st[2])]


# ---------------------------------------------------------------------------------------------
# world_size 2 over gloo: the front-end's gradient exchange (train_gpt.py:1320-1321) through GradBucket.
# Each rank's backward is the oracle's (CPU-only host); rank-averaged gradients must equal the
# unsharded backward / world.
# ---------------------------------------------------------------------------------------------
def _grad_case():
    bpt, Vt, D, Db, B, T = 8, 300, 64, 8, 4, 40
    tab = gi.synth_ttb(5101, Vt, bpt, "left").astype(np.float32)
    toks = gi.fineweb_like_tokens(5100, B, T, vocab=Vt, eot_p=0.02)
    Et, Eb = gi.normal_table(5102, Vt, D), gi.normal_table(5103, gi.BYTE_VOCAB, Db)
    g = np.random.RandomState(5104).standard_normal((B, T, D))
    pulled = orc.pull_from_left(orc.tokens_to_bytes(toks, tab), bpt, gi.PAD, gi.EOT)
    return bpt, toks, pulled, Et.astype(np.float64), Eb.astype(np.float64), g


def _grad_worker(rank, world, port, tmp):
    sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mixture_of_tokenizers_amd.grad_sync import GradBucket
    bpt, toks, pulled, Et, Eb, g = _grad_case()
    rows = slice(rank * toks.shape[0] // world, (rank + 1) * toks.shape[0] // world)
    tok_p, byte_p = torch.nn.Parameter(torch.from_numpy(Et)), torch.nn.Parameter(torch.from_numpy(Eb))
    tied = tok_p                                                  # a tied weight shows up twice in parameters()
    bucket = GradBucket([tok_p, byte_p, tied])
    assert len(bucket.params) == 2 and tok_p.grad.data_ptr() == bucket.flat.data_ptr()
    for step in range(2):                                         # the views survive zero_() and accumulate in place
        bucket.zero_()
        ref = orc.embed_mix_bwd(toks[rows], pulled[rows], None, Et, Eb, g[rows], mode="sum", bpt=bpt, norm_out=True, dtype=np.float64)
        tok_p.grad += torch.from_numpy(ref["tok_table"])
        byte_p.grad += torch.from_numpy(ref["byte_table"])
        work = bucket.all_reduce(async_op=True)
        work.wait()
    if rank == 0:
        torch.save(dict(tok=tok_p.grad.clone(), byte=byte_p.grad.clone()), tmp)
    dist.barrier()
    dist.destroy_process_group()


def test_grad_bucket_world_size_2_gloo(tmp_path):
    out = tmp_path / "g2.pt"
    port = 31500 + os.getpid() % 2000
    mp.spawn(_grad_worker, args=(2, port, str(out)), nprocs=2, join=True)
    res = torch.load(out)
    bpt, toks, pulled, Et, Eb, g = _grad_case()
    ref = orc.embed_mix_bwd(toks, pulled, None, Et, Eb, g, mode="sum", bpt=bpt, norm_out=True, dtype=np.float64)
    np.testing.assert_allclose(res["tok"].numpy(), ref["tok_table"] / 2, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(res["byte"].numpy(), ref["byte_table"] / 2, rtol=1e-12, atol=1e-12)


def test_bench_self_launch_two_ranks_gloo():
    """`python3 bench.py --gpus 2` with no torchrun environment: the parent starts both ranks itself (before any GPU call),
    they rendezvous on 127.0.0.1 (gloo here: --dry-run makes no GPU call and launches no kernel), the counters are
    all-reduced and rank 0's single JSON line comes back through the parent.  Default for N > 1 is strong scaling: ONE
    256 x 2048 batch split by rows (train_gpt.py:795-805)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    for extra, per_rank_rows, global_tokens in (([], 128, 256 * 2048), (["--scaling", "weak"], 256, 2 * 256 * 2048)):
        r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1"] + extra,
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout
        j = json.loads(lines[0])
        assert j["n_gpus"] == 2 and j["dry_run"] is True and j["steps"] == 3
        assert j["scaling"] == ("weak" if extra else "strong")
        assert f"BxT={per_rank_rows}x2048 per rank" in j["config"]["workload"]
        assert j["byte_stats"]["tokens"] == global_tokens            # summed over both ranks by the all-reduce
    # under a torchrun-style environment the process is ONE rank and must not spawn: WORLD_SIZE disagreeing with --gpus is an error
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--dry-run"], env=dict(env, WORLD_SIZE="1", RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_bench_parent_makes_no_torch_import(tmp_path):
    """The spawning parent of `bench.py --gpus N` must not initialise a HIP runtime that fork + exec would hand to the ranks
    (VERDICT r2, weak #4): it does not even import torch.  Proven by poisoning `torch` for the PARENT only: a sitecustomize-style
    stub directory that raises on `import torch` is put on PYTHONPATH when MOT_TEST_POISON_PID equals the importing pid's parent
    marker; the children drop it and import the real torch."""
    import json
    import subprocess
    poison = tmp_path / "poison"
    (poison / "torch").mkdir(parents=True)
    # the stub raises only in the process whose pid is recorded in MOT_TEST_PARENT_PID (the bench parent writes nothing there: we
    # pass the pid through a wrapper below); any other process removes the stub dir from sys.path and imports the real package
    (poison / "torch" / "__init__.py").write_text(
        "import os, sys, importlib\n"
        "if os.environ.get('MOT_TEST_PARENT_PID') == str(os.getpid()):\n"
        "    raise ImportError('bench.py parent imported torch')\n"
        "sys.path[:] = [p for p in sys.path if p != os.path.dirname(os.path.dirname(__file__))]\n"
        "del sys.modules['torch']\n"
        "sys.modules['torch'] = importlib.import_module('torch')\n"
        "globals().update(sys.modules['torch'].__dict__)\n")
    wrapper = tmp_path / "run_parent.py"
    wrapper.write_text(
        "import os, sys, runpy\n"
        "os.environ['MOT_TEST_PARENT_PID'] = str(os.getpid())\n"
        f"sys.argv = [{str(REPO / 'bench.py')!r}, '--gpus', '2', '--dry-run', '--steps', '2', '--warmup', '1']\n"
        f"runpy.run_path({str(REPO / 'bench.py')!r}, run_name='__main__')\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = str(poison) + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, str(wrapper)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert j["n_gpus"] == 2 and j["byte_stats"]["tokens"] == 256 * 2048


def test_bench_visible_gpus_reads_sysfs_only(monkeypatch, tmp_path):
    """visible_gpus(): KFD topology nodes with SIMDs are GPUs; *_VISIBLE_DEVICES lists cut the count; unreadable sysfs -> None."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_test", REPO / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    nodes = tmp_path / "nodes"
    for i, simd in enumerate((0, 0, 1024, 1024, 1024)):
        (nodes / str(i)).mkdir(parents=True)
        (nodes / str(i) / "properties").write_text(f"cpu_cores_count {64 if simd == 0 else 0}\nsimd_count {simd}\nmem_banks_count 1\n")
    real_path = bench.Path
    monkeypatch.setattr(bench, "Path", lambda p: nodes if str(p) == "/sys/class/kfd/kfd/topology/nodes" else real_path(p))
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    assert bench.visible_gpus() == 3
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,2")
    assert bench.visible_gpus() == 2
    monkeypatch.setattr(bench, "Path", lambda p: tmp_path / "missing" if str(p) == "/sys/class/kfd/kfd/topology/nodes" else real_path(p))
    assert bench.visible_gpus() is None


def test_bench_rank_slices_are_rows_of_the_one_global_batch():
    """Strong scaling in bench.py: rank r's tokens ARE rows [r*B/W, (r+1)*B/W) of the batch a single GPU runs (the id generators
    draw several arrays in a row, so they must always draw the whole batch and slice; found by the two-rank GPU rehearsal)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_slices", REPO / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    cpu = torch.device("cpu")
    for wl in ("c2", "c3"):
        B = bench.WORKLOADS[wl][0]
        whole = bench.make_inputs(wl, cpu, 12345, False)
        for world in (2, 4):
            parts = [bench.make_inputs(wl, cpu, 12345, False, rows=B // world, row0=r * (B // world)) for r in range(world)]
            np.testing.assert_array_equal(np.concatenate([p["toks"] for p in parts]), whole["toks"])
            if "chars" in whole:
                np.testing.assert_array_equal(np.concatenate([p["chars"] for p in parts]), whole["chars"])


def test_bench_plain_and_full_options_and_output_dump(tmp_path):
    """bench.py's argument contract (--full off by default, --steps at least 1) and dump_outputs(): the whole output when it fits
    in DUMP_BYTES, else DUMP_BYTES worth of rows at RandomState(0)-drawn ascending positions, always float32."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_dump", REPO / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", str(tmp_path)])
    assert a.full is True and a.dump_outputs == str(tmp_path)
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])

    small = torch.randn(2, 5, 8, dtype=torch.bfloat16)
    bench.dump_outputs(small, tmp_path / "small")
    got = np.load(tmp_path / "small" / "x.npy")
    assert got.dtype == np.float32 and got.shape == (2, 5, 8)
    np.testing.assert_array_equal(got, small.float().numpy())

    D = 1024
    keep = bench.DUMP_BYTES // (D * 4)
    big = torch.arange(3 * keep, dtype=torch.float32)[:, None].expand(3 * keep, D).reshape(3, keep, D)
    for name in ("big1", "big2"):
        bench.dump_outputs(big, tmp_path / name)
    got = np.load(tmp_path / "big1" / "x.npy")
    assert got.dtype == np.float32 and got.shape == (keep, D) and got.nbytes <= 64 << 20
    rows = got[:, 0].astype(np.int64)
    assert (got == rows[:, None]).all() and (np.diff(rows) > 0).all() and rows.max() < 3 * keep
    np.testing.assert_array_equal(rows, np.sort(np.random.RandomState(0).choice(3 * keep, keep, replace=False)))
    np.testing.assert_array_equal(np.load(tmp_path / "big2" / "x.npy"), got)
