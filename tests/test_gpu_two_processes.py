"""Two product processes on ONE GPU (round-4 verdict, item 5): the only multi-rank run with real kernels a one-GPU box allows.
`python -m torch.distributed.run --nproc-per-node 2`, gloo transport (RCCL refuses two ranks on one device), both ranks on cuda:0,
the real CLI (ifdefense_amd.opt_defense.main) on an uneven file (7 clouds: shards of 4 and 3) and on a directory of two files.

  * IFD_SPLIT=1 (what include/ifd.h prescribes for processes that share a device: no split clouds, so no cross-CU waits between
    workgroups whose co-residency another process could take away): the written files are byte-identical to the one-process run.
  * a member of every split cloud of ONE rank never arrives (test hook): that rank's launch ends in IFD_ERR_TIMEOUT after the
    bound instead of hanging the GPU, the status becomes an IfdError where the result is consumed, and the agreement in front of
    the all-gather stops BOTH ranks (dist.AgreedFailure) - nobody is left inside a collective.

Reference: the attack scripts shard a dataset over ranks and merge per-rank files (baselines/attack_scripts/targeted_knn_attack.py:97-174,
util/merge_attack_results.py:7-51); the restoration path itself is single-process there."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = '''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root)
if os.environ.get("DROP_ON_RANK") == os.environ.get("RANK"):
    os.environ["IFD_ENABLE_TEST_HOOKS"] = "1"
    os.environ["IFD_TEST_COOP_DROP"] = "1"
from ifdefense_amd import opt_defense
rc = opt_defense.main(sys.argv[2:], backend="gloo" if "WORLD_SIZE" in os.environ else None, device="cuda:0")
open(os.path.join(os.environ["DONE_DIR"], "done_rank%s" % os.environ.get("RANK", "0")), "w").write("ok")
sys.exit(rc)
'''


def _launch(tmp_path, nproc, cli_args, env_extra, timeout=600):
    script = tmp_path / "two_proc_cli.py"
    script.write_text(_SCRIPT)
    env = dict(os.environ, DONE_DIR=str(tmp_path), HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    for f in tmp_path.glob("done_rank*"):
        f.unlink()
    if nproc == 1:
        cmd = [sys.executable, str(script), ROOT] + cli_args
    else:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
               "--master-port", str(port), str(script), ROOT] + cli_args
    return subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=timeout, env=env)


def _clouds(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 1024, 3)).astype(np.float32)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(0.3, 1.0, size=(n, 1024, 1))).astype(np.float32)


def test_two_processes_on_one_gpu(tmp_path, np_weights):
    wpath = tmp_path / "convonet.pth"
    torch.save({k: torch.from_numpy(v) for k, v in np_weights.items()}, wpath)
    one, two = tmp_path / "one", tmp_path / "two"
    for d in (one, two):
        (d / "dir").mkdir(parents=True)
        np.savez(d / "adv7.npz", test_pc=_clouds(7, 1), test_label=np.arange(7), target_label=np.arange(7)[::-1].copy())
        np.savez(d / "dir" / "a.npz", test_pc=_clouds(5, 2), test_label=np.arange(5))
        np.savez(d / "dir" / "b.npz", test_pc=_clouds(3, 3), test_label=np.arange(3))
    common = ["--iterations=25", "--weights", str(wpath), "--seed=5"]
    for d, nproc in ((one, 1), (two, 2)):
        for inp in ("adv7.npz", "dir"):
            r = _launch(tmp_path, nproc, ["--data_root", str(d / inp)] + common, {"IFD_SPLIT": "1"})
            assert r.returncode == 0, r.stdout + r.stderr
            assert len(list(tmp_path.glob("done_rank*"))) == nproc
    pairs = [("ConvONet-Opt/convonet_opt-adv7.npz",) * 2, ("dir/ConvONet-Opt/convonet_opt-a.npz",) * 2, ("dir/ConvONet-Opt/convonet_opt-b.npz",) * 2]
    for a, b in pairs:
        za, zb = np.load(one / a), np.load(two / b)
        assert sorted(za.files) == sorted(zb.files)
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and np.array_equal(za[k], zb[k]), (a, k)      # two ranks on one GPU == one process, bitwise
        assert (one / a).read_bytes() == (two / b).read_bytes()
    # a split cloud's member of rank 1 never arrives: bounded wait -> IFD_ERR_TIMEOUT -> IfdError on rank 1 -> AgreedFailure on both
    t0 = time.time()
    r = _launch(tmp_path, 2, ["--data_root", str(two / "adv7.npz")] + common, {"IFD_SPLIT": "4", "IFD_COOP_TIMEOUT_MS": "50", "DROP_ON_RANK": "1"})
    dt = time.time() - t0
    out = r.stdout + r.stderr
    print("rank 1's split launch timed out: both ranks stopped after %.1f s" % dt)
    assert r.returncode != 0 and not list(tmp_path.glob("done_rank*")), out
    assert "rank 1 failed on" in out and "-5" in out and "rank 0 stops: another rank failed" in out, out
    assert dt < 120, dt


def test_bench_line_with_two_ranks_on_one_gpu(tmp_path):
    """bench.py's N > 1 code path with real kernels (round 6): two ranks under the driver's launch line, gloo transport and both ranks on
    cuda:0 (test-only flags; RCCL refuses two ranks on one device).  The weak-scaling line carries the STRONG-scaling figure too (one
    array of --clouds clouds sharded over the ranks: BASELINE configs #3 / #5), both timed with barriers on both sides and the max over
    the ranks."""
    import json
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", IFD_SPLIT="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "bench.py", "--gpus", "2", "--clouds", "40", "--steps", "2", "--warmup", "1", "--full",
           "--no-cpu-baseline", "--no-extras", "--backend", "gloo", "--device", "cuda:0"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    assert line["config"]["clouds_total"] == 80 and line["config"]["clouds_per_gpu"] == 40
    st = line["strong_scaling"]
    assert st["scaling"] == "strong" and st["clouds_total"] == 40 and st["clouds_per_gpu"] == 20 and st["value"] > 0
    print("two ranks on one GPU: weak %.1f clouds/s (80 clouds), strong %.1f clouds/s (40 clouds)" % (line["value"], st["value"]))
