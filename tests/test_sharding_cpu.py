"""Multi-GPU path on CPU: world_size 2, gloo backend, kernels replaced by the oracle-backed `_C`
stand-in.  Checks the sharding logic itself: band split, band rendering, image assembly and the
single flattened gradient all-reduce give every rank the same result as one unsharded render."""
import os

import numpy as np
import pytest
import torch as th
import torch.distributed as dist
import torch.multiprocessing as mp

from harness import free_port


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import dmesh_renderer_amd as dmr
        from dmesh_renderer_amd import scenes, sharding
        import oracle_C
        H, W, B = 88, 72, 2
        d = scenes.layered_sheets(3, 7, B, H, W, seed=1)
        gc, gd = scenes.upstream_grads(B, H, W)
        leaves = {k: d[k].clone().requires_grad_(True) for k in ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")}
        r = sharding.ShardedTriRenderer(dmr.TriRenderSettings(H, W, d["bg"]), assemble=True, impl=oracle_C, partition="bands")
        # work-balanced bands from one full render's per-tile list lengths
        full = oracle_C.render_tris(*scenes.c_args(d), H, W)
        st = oracle_C._state(full[3])[1]
        gy, gx = sharding.tile_rows(H), (W + 15) // 16
        r.set_row_work(sharding.row_work_from_ranges(st.get("ranges"), B, gy, gx))
        bands = r.bands
        color, depth = r(leaves["verts"], d["faces"], leaves["verts_color"], leaves["faces_opacity"],
                         d["mv_mats"], d["proj_mats"], leaves["verts_depth"], leaves["faces_intense"])
        ((color * gc).sum() + (depth * gd).sum()).backward()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), color=color.detach().numpy(), depth=depth.detach().numpy(),
                 bands=np.array(bands), **{"g_" + k: v.grad.numpy() for k, v in leaves.items()})
    finally:
        dist.destroy_process_group()


def test_two_rank_band_sharding(tmp_path, oracle):
    world = 2
    mp.spawn(_worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    import oracle_C
    from dmesh_renderer_amd import scenes
    H, W, B = 88, 72, 2
    d = scenes.layered_sheets(3, 7, B, H, W, seed=1)
    gc, gd = scenes.upstream_grads(B, H, W)
    args = scenes.c_args(d)
    full = oracle_C.render_tris(*args, H, W)
    gfull = oracle_C.render_tris_backward(*args, gc, gd, full[0], *full[3:7])
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert np.array_equal(r0["bands"], r1["bands"])
    b = r0["bands"]
    assert b[0][0] == 0 and b[0][1] == b[1][0] and b[1][1] == (H + 15) // 16 and b[0][1] > 0
    for r in (r0, r1):  # every rank holds the assembled image and the summed gradients
        assert np.array_equal(r["color"], full[1].numpy()) and np.array_equal(r["depth"], full[2].numpy())
        for k, g in zip(("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense"), gfull):
            assert np.abs(r["g_" + k] - g.numpy()).max() <= 1e-5 * max(1.0, float(g.abs().max())), k
    for k in ("g_verts", "g_faces_opacity"):
        assert np.array_equal(r0[k], r1[k])


def _view_worker(rank, world, port, out_dir):
    """The "view_bands" partition: B = 2 views on `world` ranks (2: one view per rank; 4: two bands per view; 3: the middle
    rank's share straddles the view border -- two segments, two B = 1 calls)."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import dmesh_renderer_amd as dmr
        from dmesh_renderer_amd import scenes, sharding
        import oracle_C
        H, W, B = 88, 72, 2
        d = scenes.layered_sheets(3, 7, B, H, W, seed=1)
        gc, gd = scenes.upstream_grads(B, H, W)
        full = oracle_C.render_tris(*scenes.c_args(d), H, W)
        st = oracle_C._state(full[3])[1]
        gy, gx = sharding.tile_rows(H), (W + 15) // 16
        res = {}
        for assemble in (True, False):
            leaves = {k: d[k].clone().requires_grad_(True) for k in ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")}
            r = sharding.ShardedTriRenderer(dmr.TriRenderSettings(H, W, d["bg"]), assemble=assemble, impl=oracle_C)  # "auto"
            r.set_row_work(sharding.view_row_work_from_ranges(st.get("ranges"), B, gy, gx))
            parts = r.view_parts(B, d["faces"].shape[0])
            assert r._use_view_bands(B) and len(parts) == world
            if world == 3:
                assert [len(p) for p in parts] == [1, 2, 1] and [v for v, _, _ in parts[1]] == [0, 1]
            else:
                assert all(len(p) == 1 for p in parts) and [p[0][0] for p in parts] == [k // (world // B) for k in range(world)]
            covered = np.zeros((B, gy), dtype=np.int64)  # the shares tile the (view, row) sequence exactly once
            for sh in parts:
                for v, a, b in sh:
                    covered[v, a:b] += 1
            assert (covered == 1).all()
            color, depth = r(leaves["verts"], d["faces"], leaves["verts_color"], leaves["faces_opacity"],
                             d["mv_mats"], d["proj_mats"], leaves["verts_depth"], leaves["faces_intense"])
            ((color * gc).sum() + (depth * gd).sum()).backward()
            tag = "a" if assemble else "s"
            res.update({tag + "_color": color.detach().numpy(), tag + "_depth": depth.detach().numpy(),
                        **{tag + "_g_" + k: v.grad.numpy() for k, v in leaves.items()}})
        np.savez(os.path.join(out_dir, f"view{rank}.npz"), segs=np.array(parts[rank], dtype=np.int64).reshape(-1, 3), **res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_view_band_sharding(tmp_path, oracle, world):
    """with B views, (view, band) segments -- the rows of all views cut into `world` contiguous shares, every
    segment rendered with B = 1 tensors; one all-gather assembles the images, ONE all-reduce over the all-views flat buffer
    sums the gradients (a rank's per-view gradients are its views' rows, zero elsewhere).  Every rank ends with the unsharded result."""
    mp.spawn(_view_worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    import oracle_C
    from dmesh_renderer_amd import scenes
    H, W, B = 88, 72, 2
    d = scenes.layered_sheets(3, 7, B, H, W, seed=1)
    gc, gd = scenes.upstream_grads(B, H, W)
    args = scenes.c_args(d)
    full = oracle_C.render_tris(*args, H, W)
    gfull = oracle_C.render_tris_backward(*args, gc, gd, full[0], *full[3:7])
    names = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")
    for rank in range(world):
        r = np.load(tmp_path / f"view{rank}.npz")
        assert np.array_equal(r["a_color"], full[1].numpy()) and np.array_equal(r["a_depth"], full[2].numpy())
        assert len(r["segs"]) >= 1
        for v, b0, b1 in r["segs"]:  # not assembled: its bands of its views
            y0, y1 = 16 * int(b0), min(H, 16 * int(b1))
            assert np.array_equal(r["s_color"][v, :, y0:y1], full[1].numpy()[v, :, y0:y1])
            assert np.array_equal(r["s_depth"][v][..., y0:y1, :], full[2].numpy()[v][..., y0:y1, :])
        for tag in ("a", "s"):
            for k, g in zip(names, gfull):
                assert np.abs(r[f"{tag}_g_{k}"] - g.numpy()).max() <= 1e-5 * max(1.0, float(g.abs().max())), (tag, k)


def _tet_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import dmesh_renderer_amd as dmr
        from dmesh_renderer_amd import scenes, sharding
        import oracle_C
        H, W, B = 88, 72, 2
        d = scenes.kuhn_tets(3, B, H, W, seed=2)
        gc, gd = scenes.upstream_grads(B, H, W)
        vc = d["verts_color"].clone().requires_grad_(True); fo = d["faces_opacity"].clone().requires_grad_(True)
        r = sharding.ShardedTetRenderer(dmr.TetRenderSettings(H, W, d["bg"], 0), assemble=True, impl=oracle_C)
        r.bands = [(0, 2), (2, sharding.tile_rows(H))]  # unequal bands: 2 and 4 tile rows
        color, depth, active = r(d["verts"], d["faces"], vc, fo, d["mv_mats"], d["proj_mats"], d["verts_depth"],
                                 d["faces_intense"], d["tets"], d["face_tets"], d["tet_faces"])
        ((color * gc).sum() + (depth * gd).sum()).backward()
        np.savez(os.path.join(out_dir, f"tet{rank}.npz"), color=color.detach().numpy(), depth=depth.detach().numpy(),
                 active=active.numpy(), g_vc=vc.grad.numpy(), g_fo=fo.grad.numpy())
    finally:
        dist.destroy_process_group()


def test_two_rank_tet_band_sharding(tmp_path, oracle):
    """ShardedTetRenderer ("the tet path shards identically"): bands of the march, one all-gather of the
    three images, ONE all-reduce over [3P | F] -- every rank ends with the unsharded result."""
    world = 2
    mp.spawn(_tet_worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    import oracle_C
    from dmesh_renderer_amd import scenes
    H, W, B = 88, 72, 2
    d = scenes.kuhn_tets(3, B, H, W, seed=2)
    gc, gd = scenes.upstream_grads(B, H, W)
    args = scenes.c_args(d, tet=True)
    full = oracle_C.render_tets(*args, H, W, 0)
    gfull = oracle_C.render_tets_backward(*args, gc, gd, *full[3:7])
    assert full[2].sum() > 0
    for k in range(world):
        r = np.load(tmp_path / f"tet{k}.npz")
        assert np.array_equal(r["color"], full[0].numpy()) and np.array_equal(r["depth"], full[1].numpy())
        assert np.array_equal(r["active"], full[2].numpy() > 0.5)
        for key, g in (("g_vc", gfull[0]), ("g_fo", gfull[1])):
            assert np.abs(r[key] - g.numpy()).max() <= 1e-5 * max(1.0, float(g.abs().max())), key


def test_band_helpers():
    from dmesh_renderer_amd import sharding
    assert sharding.equal_bands(68, 8)[0] == (0, 8) and sharding.equal_bands(68, 8)[-1][1] == 68
    w = np.zeros(68); w[20:48] = 100.0
    bands = sharding.balanced_bands(w, 4)
    assert bands[0][0] == 0 and bands[-1][1] == 68
    loads = [w[a:b].sum() for a, b in bands]
    assert max(loads) <= 1.3 * (w.sum() / 4)
    assert all(bands[i][1] == bands[i + 1][0] for i in range(3))
    g = [th.arange(6.).reshape(2, 3), th.arange(4.)]
    flat = sharding.flatten_grads(g)
    back = sharding.unflatten_grads(flat, g)
    assert all(th.equal(a, b_) for a, b_ in zip(g, back))


def test_band_balance_counts_tiles_as_well_as_list_entries():
    """`row_work_from_ranges`: a band's cost is its list entries plus a cost per tile (sharding.TILE_COST_ENTRIES, measured at
    C5: profiles/r03/shard_kernel_sums_c5*.json).  A frame whose entries sit in the middle rows: balanced by entries alone the
    edge bands get most of the (nearly empty) rows; with the per-tile cost they give rows up, every band still holds work, and
    the bands still partition the rows."""
    from dmesh_renderer_amd import sharding
    B, gy, gx = 2, 64, 48
    lens = np.zeros((B, gy, gx), dtype=np.int64)
    lens[:, 24:40, 8:40] = 200            # a dense patch in the middle rows
    lens[:, :, 20:28] += 3                # a thin column everywhere
    ends = np.cumsum(lens.reshape(-1))
    ranges = np.stack([ends - lens.reshape(-1), ends], axis=1)
    world = 8
    by_entries = sharding.balanced_bands(sharding.row_work_from_ranges(ranges, B, gy, gx, tile_cost=0.0), world)
    by_cost = sharding.balanced_bands(sharding.row_work_from_ranges(ranges, B, gy, gx), world)
    for bands in (by_entries, by_cost):
        assert bands[0][0] == 0 and bands[-1][1] == gy and all(a[1] == b[0] for a, b in zip(bands[:-1], bands[1:]))
    rows = lambda bands: [b[1] - b[0] for b in bands]
    assert rows(by_cost)[0] < rows(by_entries)[0] and rows(by_cost)[-1] < rows(by_entries)[-1]
    cost = lambda b: lens[:, b[0]:b[1]].sum() + sharding.TILE_COST_ENTRIES * B * gx * (b[1] - b[0])
    spread = lambda bands: max(cost(b) for b in bands) / (sum(cost(b) for b in bands) / world)
    assert spread(by_cost) < spread(by_entries)


def test_view_shares_balance_unequal_views():
    """`view_shares`: contiguous shares of the (view, row) sequence; a share pays `segment_cost` per view it touches; the
    bisection finds the smallest maximum.  C5-like: views of work 3 : 1.6 : 3 : 1.44 on 8 ranks."""
    from dmesh_renderer_amd.sharding import view_shares
    w = np.repeat(np.array([[3.0], [1.6], [3.0], [1.44]]), 64, axis=1)
    seg = 8.0
    sh = view_shares(w, 8, seg)
    assert len(sh) == 8
    cost = [sum(w[v, a:b].sum() + seg for v, a, b in s) for s in sh]
    ideal = (w.sum() + 4 * seg) / 8
    assert max(cost) <= 1.12 * ideal, (cost, ideal)  # equal ranks per view (2 each) would give 3.0 * 32 + 8 = 104 against 72.4
    covered = np.zeros(w.shape, dtype=np.int64)
    for s in sh:
        for v, a, b in s:
            covered[v, a:b] += 1
    assert (covered == 1).all()
    # more ranks than rows: the extra shares are empty
    assert sum(1 for s in view_shares(np.ones((2, 2)), 6, 0.0) if s) == 4


def test_row_work_counts_blended_pairs_when_given():
    """With `tile_hits` (blended pairs per tile of a forward) the work of a row is entries + PAIR_COST_ENTRIES per pair +
    TILE_COST_ENTRIES_WITH_PAIRS per tile (the model fitted in profiles/r03/shard_cost_model_c5.txt): two rows with the same
    list entries but different coverage no longer weigh the same."""
    from dmesh_renderer_amd import sharding
    B, gy, gx = 1, 4, 8
    lens = np.full((B, gy, gx), 100, dtype=np.int64)
    ends = np.cumsum(lens.reshape(-1))
    ranges = np.stack([ends - lens.reshape(-1), ends], axis=1)
    hits = np.zeros((B, gy, gx), dtype=np.int64)
    hits[0, 0] = 20000  # the first row's faces cover many pixels
    w0 = sharding.view_row_work_from_ranges(ranges, B, gy, gx)
    w1 = sharding.view_row_work_from_ranges(ranges, B, gy, gx, tile_hits=hits)
    assert w0.shape == w1.shape == (B, gy) and np.allclose(w0[0], w0[0, 0])
    assert np.isclose(w1[0, 1], 100 * gx + sharding.TILE_COST_ENTRIES_WITH_PAIRS * gx)
    assert np.isclose(w1[0, 0] - w1[0, 1], sharding.PAIR_COST_ENTRIES * 20000 * gx)
    assert np.allclose(sharding.row_work_from_ranges(ranges, B, gy, gx, tile_hits=hits), w1.sum(axis=0))
    assert sharding.segment_cost(1000, True) > sharding.segment_cost(1000, False) > 0
