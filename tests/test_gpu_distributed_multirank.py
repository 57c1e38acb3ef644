"""GPU, world_size 2 - 4 on ONE device: rasterization(distributed=True) with the real kernels, both seams and the
autograd-generated reverse exchange, against the single-process render of the whole scene.

RCCL refuses two ranks on one GPU, so the process group is gloo (which moves the CUDA buffers through the host): what
is under test is everything around the collectives - Gaussian sharding, camera all-gather, the personalised all-to-all of
projected rows (dense: the two overlapped asynchronous messages; packed: variable-length messages), row order on the
receiving side, the gradients that travel back to the rank that owns the Gaussian - with the kernels in the loop.
Contract: reference tests/test_rasterization.py:819-868 (distributed == local on the same scene)."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("means", "quats", "scales", "opacities", "colors")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, results, packed, c_local, WORLD):
    import traceback

    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GSPLAT_AMD_ALLOW_NON_NCCL="1")
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        import gsplat_amd as G
        from _util import assert_close_ratio, assert_grad_close, make_scene

        dev = torch.device("cuda", 0)
        C = WORLD * c_local
        sc, W, H = make_scene(N=4001, C=C, width=176, height=112, seed=21, sh_degree=2)
        g = torch.Generator().manual_seed(9)
        v_rc, v_ra = torch.randn(C, H, W, 3, generator=g), torch.randn(C, H, W, 1, generator=g)
        mine = slice(rank * c_local, (rank + 1) * c_local)  # this rank's cameras
        shard = slice(rank, None, WORLD)                     # this rank's Gaussians

        # reference: ONE process renders every camera with every Gaussian. Gaussians in the order the ranks hold them
        # (rank 0's shard, then rank 1's): flatten ids - the tie-break of equal depths - then agree with the exchange.
        order = torch.cat([torch.arange(r, 4001, WORLD) for r in range(WORLD)])
        full = {k: sc[k][order].to(dev).clone().requires_grad_(True) for k in NAMES}
        rc0, ra0, _ = G.rasterization(full["means"], full["quats"], full["scales"], full["opacities"], full["colors"],
                                      sc["viewmats"].to(dev), sc["Ks"].to(dev), W, H, sh_degree=2, packed=packed)
        ((rc0 * v_rc.to(dev)).sum() + (ra0 * v_ra.to(dev)).sum()).backward()
        counts = [len(range(r, 4001, WORLD)) for r in range(WORLD)]
        rows = slice(sum(counts[:rank]), sum(counts[:rank + 1]))

        # distributed: this rank owns a shard of the Gaussians and c_local cameras
        loc = {k: sc[k][shard].to(dev).clone().requires_grad_(True) for k in NAMES}
        rc1, ra1, meta = G.rasterization(loc["means"], loc["quats"], loc["scales"], loc["opacities"], loc["colors"],
                                         sc["viewmats"][mine].to(dev), sc["Ks"][mine].to(dev), W, H, sh_degree=2,
                                         packed=packed, distributed=True)
        ((rc1 * v_rc[mine].to(dev)).sum() + (ra1 * v_ra[mine].to(dev)).sum()).backward()
        torch.cuda.synchronize()
        assert rc1.shape == (c_local, H, W, 3)
        assert_close_ratio(rc1.detach().cpu(), rc0[mine].detach().cpu(), 1e-5, 1e-5, max_bad_ratio=1e-4, name="colors")
        assert_close_ratio(ra1.detach().cpu(), ra0[mine].detach().cpu(), 1e-5, 1e-5, max_bad_ratio=1e-4, name="alphas")
        for k in NAMES:  # gradients of MY Gaussians from EVERY rank's images came back through the reverse exchange
            assert_grad_close(loc[k].grad.cpu(), full[k].grad[rows].cpu(), rel=2e-4, name=f"rank {rank} v_{k}")
        results[rank] = "ok"
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        results[rank] = traceback.format_exc()
        raise


@pytest.mark.parametrize("world,c_local,packed", [(2, 2, False), (2, 1, False), (2, 2, True), (2, 1, True), (3, 2, False),
                                                  (3, 1, True), (4, 1, False), (8, 4, False), (8, 1, True)])
def test_ranks_sharing_one_gpu_match_the_single_process_render(world, packed, c_local):
    """world 3: shards of unequal size (1334 / 1334 / 1333 Gaussians); world 4: three peers per rank; world 8: the shape of
    BASELINE.json configs[3] - seven peers per rank, shards of 501 / 500 Gaussians, four cameras per rank (32 in the job)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    mgr = mp.Manager()
    results = mgr.dict()
    ctx = mp.spawn(_worker, args=(_free_port(), results, packed, c_local, world), nprocs=world, join=False)
    ok = ctx.join(timeout=300)
    while not ok:
        ok = ctx.join(timeout=300)
    assert dict(results) == {r: "ok" for r in range(world)}, "\n".join(f"rank {r}: {m}" for r, m in dict(results).items())


def test_bench_two_rank_path_rehearsal():
    """bench.py's N > 1 path (c4-shaped: Gaussian-sharded scene, 4 cameras per rank, both seams, barriers, max over ranks,
    ONE JSON line from rank 0) launched exactly as the driver launches it, with two ranks sharing the GPU over gloo
    (GSPLAT_BENCH_REHEARSAL=1). Timings of a rehearsal mean nothing; the structure of the line is what is checked."""
    import json
    import subprocess

    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    env = dict(os.environ, GSPLAT_BENCH_REHEARSAL="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--gaussians", "60000", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["steps"] == 2 and r["warmup"] == 1 and r["scaling"] == "weak" and r["rehearsal"] is True
    assert r["config"]["cameras_per_gpu"] == 4 and r["config"]["gaussians_per_gpu"] == 60000
    assert r["config"]["parallelism"] == "gaussian-sharded x2" and r["value"] > 0 and r["unit"] == "Mpixels/s"
    assert "cpu_baseline" not in r and "roofline" in r  # the CPU baseline is an N = 1 leg
    ref = r["c4_single_gpu"]  # rank 0's single-GPU reference of the same workload, measured after the timed region
    assert ref["value"] > 0 and "120000 synthetic Gaussians" in ref["workload"] and "rank 0" in ref["note"]
    # the line rounds the ratio to three decimals: compare on that grid (0.021 against 0.02123 is not a 1 % difference)
    assert r["speedup_vs_1gpu"] == pytest.approx(r["value"] / ref["value"], rel=1e-2, abs=6e-4) and r["efficiency"] > 0


def test_bench_eight_rank_path_rehearsal():
    """`python bench.py --gpus 8` as the driver's scaling run launches it (c4: 4 cameras per rank, the scene stride-sharded
    eight ways), rehearsed with the eight ranks sharing this GPU over gloo: the line must carry the all-to-all volume per rank
    so that a real run can be checked against SURVEY.md section 8(e) (dense rows: 7 peers x C_local N_local rows x 48 B per
    direction, doubled by the reverse exchange of the 40-byte gradient rows)."""
    import json
    import subprocess

    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["GSPLAT_BENCH_REHEARSAL"] = "1"
    n_local = 5000
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--gaussians", str(n_local),
           "--no-extra", "--windows", "1", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 8 and r["rehearsal"] is True and r["value"] > 0 and r["config"]["cameras_per_gpu"] == 4
    assert r["config"]["parallelism"] == "gaussian-sharded x8" and len(r["windows_ms"]) == 2
    # forward: rows to 7 peers, 4 of their cameras each, (7 geometry + 3 colour floats + 2 radii words) = 48 B per row; backward:
    # the gradient of the 10 payload floats comes back = 40 B per row
    rows_to_peers = 7 * 4 * n_local
    assert r["a2a_bytes_per_rank"] == pytest.approx(rows_to_peers * (48 + 40), rel=0.02), r["a2a_bytes_per_rank"]


def test_bench_plain_form_launches_its_own_ranks():
    """`python bench.py --gpus 2` without a launcher (the form the driver records): bench.py re-executes itself under
    torch.distributed.run - one rank per GPU - instead of failing on WORLD_SIZE (gsplat/distributed.py:319-375 spawns its
    ranks itself too). Rehearsed with both ranks on the one GPU over gloo."""
    import json
    import subprocess

    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["GSPLAT_BENCH_REHEARSAL"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--gaussians", "40000",
           "--no-extra"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["rehearsal"] is True and r["value"] > 0


def test_bench_single_gpu_line_has_the_contract_fields():
    """The N = 1 line as the driver reads it, on a reduced scene: every contract field present and of the right kind (a
    sub-record that turns into a number, or a roofline object that loses a key, fails here instead of in the driver's parser)."""
    import json
    import subprocess

    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--gaussians", "100000", "--no-extra",
           "--no-cpu-baseline", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 1 and r["steps"] == 2 and r["warmup"] == 1 and r["higher_is_better"] is True and r["scaling"] == "weak"
    assert r["unit"] == "Mpixels/s" and r["value"] > 0 and r["ms_per_step"] > 0 and r["dtype"] == "f32" and r["data"] == "synthetic"
    assert r["vs_baseline"] is None and isinstance(r["config"], dict) and "workload" in r["config"]
    roof = r["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "valu_issue_frac"):
        assert key in roof, key
    assert roof["bound"] == "hbm" and roof["peak"] == 8000.0 and 0 < roof["frac"] < 1
    assert roof["traffic"] is None or roof["traffic"] > 0
    if roof["valu_issue"] is not None:
        assert 0 < roof["valu_issue"]["frac"] < 1 and 0 < roof["valu_issue"]["by_class"]["frac_of_launch"] < 1.5
    other = r["other_layout"]
    assert isinstance(other, dict) and other["packed"] is True and other["ms_per_step"] > 0 and other["value"] > 0
    assert isinstance(r["stage_ms_per_step"], dict) and r["raster_launch_ms"]["fwd"] > 0 and r["raster_launch_ms"]["bwd"] > 0
    # the driver-specified window first, then its repeats; the forward and the pair the north star quotes next to the backward
    assert len(r["windows_ms"]) == 7 and r["windows_ms"][0] == pytest.approx(r["ms_per_step"], rel=1e-3)
    assert r["value_best"] >= r["value_median"] > 0 and r["instrumented_window_ms"] > 0
    for view in ("fwd", "bwd", "fwd_plus_bwd"):
        assert 0 < roof[view]["frac"] < 1 and roof[view]["launch_ms"] > 0, view


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain N = 1 run times the headline window only (no roofline, repeats or sub-records) and `--dump-outputs` writes what
    its last timed step computed: the image, as rendered again here from the same seeded workload, and sampled gradients."""
    import json
    import subprocess

    import numpy as np

    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    n = 100000
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--gaussians", str(n),
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "Mpixels/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(1920 * 1080 / (r["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    for key in ("roofline", "windows_ms", "other_layout", "c5", "c4_single_gpu", "cpu_baseline", "stage_ms_per_step"):
        assert key not in r, key
    files = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(files) == {"render_colors", "render_alphas", "grad_means", "grad_quats", "grad_scales", "grad_opacities",
                          "grad_colors"}
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["render_colors"].shape == (1, 1080, 1920, 3) and files["render_alphas"].shape == (1, 1080, 1920, 1)
    assert files["grad_means"].shape == (1 << 16, 3) and files["grad_colors"].shape == (1 << 16, 16, 3)
    assert np.isfinite(files["grad_colors"]).all() and np.abs(files["grad_colors"]).sum() > 0

    sys.path.insert(0, ROOT)
    import bench
    import gsplat_amd

    sc, W, H = bench.make_workload(n, "cuda")
    leaves = {k: sc[k].clone().requires_grad_(True) for k in NAMES}
    rc, ra, _ = gsplat_amd.rasterization(*(leaves[k] for k in NAMES), sc["viewmats"], sc["Ks"], W, H, sh_degree=3, packed=False,
                                         tile_size=bench.TILE)
    np.testing.assert_allclose(files["render_colors"], rc.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(files["render_alphas"], ra.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
