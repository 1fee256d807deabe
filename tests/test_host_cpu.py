"""CPU: host logic of the drop-in boundary (no compute calls without a GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import refnerf_pl_amd  # noqa: F401
from refnerf_pl_amd import _hip, configs, layout, models, synthetic, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIN = os.path.join(ROOT, "configs", "refnerf_blender.gin")


@pytest.fixture()
def cfg():
    configs.clear_config()
    configs.parse_config_files_and_bindings([GIN], [])
    yield configs.Config()
    configs.clear_config()


def test_library_exports_every_declared_symbol():
    """The C-ABI library loads and exports exactly what include/refnerf_hip.h declares."""
    hdr = open(os.path.join(ROOT, "include", "refnerf_hip.h")).read()
    names = set(re.findall(r"\b(refnerf_[a-z_0-9]+)\s*\(", hdr))
    from refnerf_pl_amd import _abi
    assert names == set(_abi.prototypes)            # the binding's parser (which _hip.lib() binds from) drops no declaration
    assert {"refnerf_level_forward", "refnerf_pack_weights", "refnerf_sample_intervals",
            "refnerf_integrated_pos_enc", "refnerf_integrated_dir_enc"} <= names
    lib = _hip.lib()
    for n in names:
        assert hasattr(lib, n), n
    assert lib.refnerf_abi_version() == 11
    assert _hip.packed_weights_bytes(_hip.PREC_F32) > 4 * layout.NUM_PARAMS
    # 17 KB chunks (+ 2 chunks of tail pad the ring may prefetch into): 150 for the plain 16-bit images, 206 for the split-f16 one
    # (133 spatial + heads chunks on the 16x16x32 layout, streamed twice per pass, + 73 directional: refnerf_layout.h)
    assert _hip.packed_weights_bytes(_hip.PREC_BF16) == _hip.packed_weights_bytes(_hip.PREC_F16) == 152 * 17408
    assert _hip.packed_weights_bytes(_hip.PREC_F16X2) == 208 * 17408
    c = _hip.default_cfg()
    assert (c.n_samples, c.resample_padding, c.density_bias) == (128, pytest.approx(0.01), pytest.approx(0.5))
    assert C.sizeof(_hip.LevelCfg) == 100 and c.ipe_groups == 0 and _hip.lib().refnerf_packed_weights_bytes_basis(_hip.PREC_F32, 7) > 4 * _hip.NUM_PARAMS_EXT and c.dir_enc == _hip.DIRENC_IDE and c.raydist == 0 and c.disable_integration == 0 and c.wgrad_mode == _hip.WGRAD_BF16X3 and C.sizeof(_hip.LevelOut) == 23 * 8


def test_gin_loader_syntax(tmp_path):
    configs.clear_config()
    f = tmp_path / "x.gin"
    f.write_text("# comment\nConfig.exp_name = \\\n    'a#b'\nModel.num_levels = 2  # trailing\n"
                 "Config.near = 0.\nNerfMLP.basis_shape = 'octahedron'\nConfig.unknown_field = 3\n")
    configs.parse_config_files_and_bindings([str(f)], ["Config.batch_size = 77", "train/Config.far = 9."])
    c = configs.Config()
    assert (c.exp_name, c.near, c.batch_size, c.far) == ("a#b", 0.0, 77, 9.0)
    assert configs.bindings_for("Model") == {"num_levels": 2}
    assert "Model.num_levels = 2" in configs.config_str()
    configs.clear_config()


def test_model_surface_and_state_dict(cfg):
    model = models.construct_model(utils.dummy_rays(), cfg)
    assert isinstance(model.nerf_mlp, models.NerfMLP) and model.prop_mlp is model.nerf_mlp
    sd = model.state_dict()
    assert len(sd) == 92                                   # 46 tensors, aliased under prop_mlp
    assert sum(p.numel() for p in model.parameters()) == layout.NUM_PARAMS
    for spec in layout.PARAM_SPECS:
        for pre in ("nerf_mlp.", "prop_mlp."):
            assert tuple(sd[pre + spec.name + ".weight"].shape) == (spec.out_dim, spec.in_dim)
            assert tuple(sd[pre + spec.name + ".bias"].shape) == (spec.out_dim,)
    # reference init: U(+-1/sqrt(fan_in)), zero bias (models.py:38-47)
    w = model.nerf_mlp.spatial_net[1].weight
    assert float(w.abs().max()) <= 1 / 16 + 1e-6 and float(model.nerf_mlp.rgb.bias.abs().max()) == 0
    assert (model.num_levels, model.num_prop_samples, model.num_nerf_samples, model.single_mlp) == (2, 128, 128, True)


def test_flat_params_alias_and_roundtrip(cfg):
    mlp = models.construct_model(None, cfg).nerf_mlp
    blob = synthetic.make_params(3, 0.1)
    mlp.load_flat_params(blob)
    flat = mlp.flat_params()
    assert np.array_equal(flat.numpy(), blob)
    spec = layout.SPEC_BY_NAME["viewdir_mlp.5"]
    assert np.array_equal(mlp.viewdir_mlp[5].weight.detach().numpy().reshape(-1), blob[spec.w_off:spec.w_off + 256 * 457])
    with torch.no_grad():
        mlp.rgb.bias.add_(1.0)                              # an optimiser-style in-place update
    assert flat[layout.SPEC_BY_NAME["rgb"].b_off].item() == pytest.approx(blob[layout.SPEC_BY_NAME["rgb"].b_off] + 1.0)
    sd = mlp.state_dict()
    mlp2 = models.NerfMLP()
    mlp2.load_state_dict(sd)
    assert np.array_equal(mlp2.flat_params().numpy(), flat.numpy())


def test_unsupported_configurations_raise(cfg):
    with pytest.raises(ValueError, match="the reference itself cannot run"):
        models.MLP()                                        # reference defaults = mip-NeRF MLP (dead in the reference too)
    with pytest.raises(ValueError, match="Normals must be computed"):   # models.py:472-475
        models.MLP(use_reflections=True, enable_pred_normals=False, disable_density_normals=True)
    with pytest.raises(ValueError, match="Specular density is useless"):  # models.py:478-480
        models.MLP(enable_pred_specular_density=True, use_diffuse_color=False)
    with pytest.raises(ValueError, match="outside the fused"):
        models.Model(config=cfg, use_viewdirs=False)
    with pytest.raises(KeyError):                          # coord.py:92: inv_mapping[fn.__name__]
        models.Model(config=cfg, raydist_fn=torch.tanh)
    m = models.Model(config=cfg, raydist_fn="@torch.reciprocal", disable_integration=True)     # built (cfg.raydist, cfg.disable_integration)
    assert m._raydist_code == _hip.RAYDIST["reciprocal"] and models.Model._raydist_enum(torch.log) == 3 and models.Model._raydist_enum("piecewise") == 1
    assert models.Model(config=cfg, dilation_bias=0.0025).dilation_bias == 0.0025      # built (host dilation)


def test_specular_density_head_module_matches_the_reference(cfg):
    """NerfMLP.enable_pred_specular_density: the module gains `raw_specular_density` where the reference's has it (state_dict names
    and order captured from the reference: tests/golden/model_specdens_eval.npz), outside the canonical 46-tensor blob the kernels
    take; a state_dict round trip carries it."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "model_specdens_eval.npz"))
    mlp = models.NerfMLP(enable_pred_specular_density=True)
    assert list(mlp.state_dict().keys()) == [str(k) for k in g["state_dict_keys"]]
    assert tuple(mlp.raw_specular_density.weight.shape) == (1, 256) and mlp.num_params == layout.NUM_PARAMS
    with torch.no_grad():
        mlp.raw_specular_density.weight.copy_(torch.tensor(g["specdens_w"]))
    mlp2 = models.NerfMLP(enable_pred_specular_density=True)
    mlp2.load_state_dict(mlp.state_dict())
    assert torch.equal(mlp2.raw_specular_density.weight, mlp.raw_specular_density.weight)
    assert np.array_equal(mlp2.flat_params().detach().numpy(), mlp.flat_params().detach().numpy())
    with pytest.raises(RuntimeError):                       # a module without the head does not take the extra tensors silently
        models.NerfMLP().load_state_dict(mlp.state_dict())


def test_variant_gate_matches_reference_status():
    """what the reference itself survives (tests/golden/variants_status.json, captured by
    make_golden.py `variants`) against this build's gate.  Both shipped mip-NeRF configs and the flag settings behind them
    die inside the reference; every single flag it does run is served (the icosahedron basis as direction groups: tests/test_basis.py)."""
    import json
    st = json.load(open(os.path.join(ROOT, "tests", "golden", "variants_status.json")))
    assert st["configs"]["blender_mipnerf.gin"].startswith("KeyError: 'diffuse'")
    assert st["configs"]["llff_mipnerf.gin"].startswith("KeyError: 'diffuse'")
    assert all(v == "ok" for k, v in st["configs"].items() if "mipnerf" not in k)
    not_built = set()
    ref_cfg = os.path.join(ROOT, "configs", "refnerf_blender.gin")
    for flag, status in st["refnerf_with_flag"].items():
        configs.clear_config()
        configs.parse_config_files_and_bindings([ref_cfg], [flag])
        if status != "ok":
            with pytest.raises(ValueError, match="the reference itself cannot run"):
                models.NerfMLP()
        elif flag in not_built:
            with pytest.raises(ValueError, match="outside the fused Ref-NeRF family"):
                models.NerfMLP()
        else:
            mlp = models.NerfMLP()
            name, val = flag.split(" = ")
            assert str(getattr(mlp, name.split(".")[1])) == val.strip("'")
    configs.clear_config()


def test_variant_embedding_layout():
    """layout.variant_layout: true shapes of the reference's modules, a one-to-one map into the canonical blob, zeros
    elsewhere; the module exposes exactly the reference's parameter names."""
    specs, idx = layout.variant_layout(128, False, False, False)
    shapes = {s.name: (s.out_dim, s.in_dim) for s in specs}
    assert "raw_tint" not in shapes and "raw_roughness" not in shapes
    assert shapes["viewdir_mlp.0"] == (128, 200) and shapes["viewdir_mlp.5"] == (128, 328) and shapes["rgb"] == (3, 128)
    assert shapes["spatial_net.5"] == (256, 352) and shapes["bottleneck"] == (128, 256)
    assert len(set(idx.tolist())) == len(idx) == specs[-1].b_off + 3 and idx.max() < layout.NUM_PARAMS
    assert layout.variant_layout()[1] is None
    mlp = models.MLP(net_depth_viewdirs=8, net_width_viewdirs=128, bottleneck_width=128, max_deg_point=16, deg_view=5,
                     use_reflections=True, use_directional_enc=True, enable_pred_roughness=False, use_diffuse_color=True,
                     use_specular_tint=False, use_n_dot_v=False, enable_pred_normals=True, basis_shape="octahedron",
                     basis_subdivisions=1)
    names = [n for n, _ in mlp.named_parameters()]
    assert "raw_tint.weight" not in names and "raw_roughness.weight" not in names
    assert tuple(mlp.viewdir_mlp[5].weight.shape) == (128, 328)
    blob = synthetic.make_params(seed=3)
    mlp.load_flat_params(blob)                               # canonical blob in: the embedded elements are taken
    canon = mlp.canonical_blob().numpy()
    assert np.array_equal(canon[idx], blob[idx])
    rest = np.ones(layout.NUM_PARAMS, bool)
    rest[idx] = False
    assert not canon[rest].any()
    assert mlp.kernel_roughness_bias == layout.ROUGHNESS_OFF_BIAS


def test_no_cpu_fallback(cfg):
    """Without a GPU the product path must fail loudly, never fall back."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    model = models.construct_model(None, cfg).eval()
    rays = utils.rays_from_dict(synthetic.blender_rays(4))
    rays.to("cpu")
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        model(rays, 1.0, False)
    with pytest.raises(_hip.HipLibraryError):
        _hip.pack_weights(torch.zeros(layout.NUM_PARAMS))


def test_product_never_imports_oracle():
    """oracle/ is test infrastructure: the product may not import, link, load or include it."""
    pat = re.compile(r"(from\s+oracle|import\s+oracle|librefnerf_oracle|#include\s*[\"<][^\n]*oracle)")
    pkg = os.path.join(ROOT, "refnerf-pl_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")) or fn == "Makefile":
                assert not pat.search(open(os.path.join(dirpath, fn)).read()), fn


def test_rays_container():
    r = utils.rays_from_dict(synthetic.blender_rays(10))
    assert r.shape == (10, 3) and r[2:5].origins.shape == (3, 3)
    r.to("cpu")
    assert isinstance(r.origins, torch.Tensor) and r.origins.dtype == torch.float32
    assert r.reshape(2, 5, -1).radii.shape == (2, 5, 1)
    d = utils.dummy_rays()
    assert d.cam_idx.dtype == torch.int32 and d.origins.shape == (1, 3)


def test_synthetic_ray_statistics():
    b = synthetic.blender_rays(512, seed=1)
    nd = np.linalg.norm(b["directions"], axis=-1)
    assert 1.0 <= nd.min() and nd.max() < 1.12
    np.testing.assert_allclose(b["radii"], 5.196e-4, rtol=2e-2)
    np.testing.assert_allclose(np.linalg.norm(b["viewdirs"], axis=-1), 1.0, atol=1e-6)
    l = synthetic.llff_rays(512, seed=1)
    assert np.allclose(l["origins"][:, 2], -1.0) and np.allclose(l["directions"][:, 2], 2.0)
    assert np.array_equal(synthetic.make_params(5, 0.1), synthetic.make_params(5, 0.1))


@pytest.mark.parametrize("name,extra", [("model_blender_sharp_train", []),
                                        ("model_llff_linear_train", None)])
def test_losses_match_reference_values(cfg, name, extra):
    """train_utils mirror (a18-a20): evaluated on the reference's own level
    outputs (golden fixtures) it reproduces the reference's loss values, and its
    gradients w.r.t. rgb / weights / normals_pred exist (what the HIP backward consumes)."""
    import sys
    sys.path.insert(0, os.path.dirname(__file__))
    from helpers import load_golden, rays_from_golden
    from refnerf_pl_amd import train_utils
    g = load_golden(name)
    rays = utils.rays_from_dict(rays_from_golden(g))
    batch = utils.Batch(rays=rays, rgb=np.asarray(g["gt_rgb"], np.float32))
    rend, hist = [], []
    for L in range(2):
        rend.append({"rgb": torch.tensor(g[f"L{L}_r_rgb"], requires_grad=True)})
        hist.append({"weights": torch.tensor(g[f"L{L}_h_weights"], requires_grad=True),
                     "normals": torch.tensor(g[f"L{L}_h_normals"]),
                     "normals_pred": torch.tensor(g[f"L{L}_h_normals_pred"], requires_grad=True)})

    class M:
        num_levels = 2
    total, terms, stats = train_utils.compute_losses(M, batch, rays, rend, hist, cfg)
    assert float(terms["data"].detach()) == pytest.approx(float(g["loss_data"]), rel=1e-6)
    assert float(terms["orientation"].detach()) == pytest.approx(float(g["loss_orientation"]), rel=1e-5)
    assert float(terms["predicted_normals"].detach()) == pytest.approx(float(g["loss_normal"]), rel=1e-5)
    assert float(total.detach()) == pytest.approx(float(g["loss_total"]), rel=1e-6)
    total.backward()
    for L in range(2):
        assert rend[L]["rgb"].grad is not None and hist[L]["weights"].grad is not None
        assert hist[L]["normals_pred"].grad is not None
    hist[0]["normals"] = None
    with pytest.raises(ValueError):
        train_utils.predicted_normal_loss(M, hist, cfg)


def test_image_writers_match_reference_pixels(tmp_path):
    """save_img_u8 (plain and masked) / save_img_f32 / write_render_outputs: decoded pixels equal the
    reference's writers on the same arrays (tests/golden/io.npz)."""
    from PIL import Image
    from refnerf_pl_amd import utils
    g = np.load(os.path.join(ROOT, "tests", "golden", "io.npz"))
    utils.save_img_u8(torch.tensor(g["img"]), str(tmp_path / "a.png"))
    assert np.array_equal(np.array(Image.open(tmp_path / "a.png")), g["png_rgb"])
    utils.save_img_u8(g["rough"], str(tmp_path / "b.png"), mask=torch.tensor(g["acc"]))
    assert np.array_equal(np.array(Image.open(tmp_path / "b.png")), g["png_rho_masked"])
    utils.save_img_f32(g["depth"], str(tmp_path / "c.tiff"))
    assert np.array_equal(utils.load_img(str(tmp_path / "c.tiff")), g["tiff_depth"])
    rendering = {"rgb": g["img"], "diffuse": g["img"], "specular": g["img"], "normals_pred": g["img"] * 2 - 1,
                 "acc": g["acc"], "distance_mean": g["depth"], "distance_median": g["depth"], "roughness": g["rough"],
                 "tint": g["img"]}
    paths = utils.write_render_outputs(rendering, str(tmp_path / "out"), 7)
    assert sorted(os.path.basename(p) for p in paths) == sorted(
        [f"{n}_007.png" for n in ("color", "diffuse", "specular", "normals_pred", "rho")] +
        [f"{n}_007.tiff" for n in ("distance_mean", "distance_median", "acc")])
    assert np.array_equal(np.array(Image.open(tmp_path / "out" / "rho_007.png")), g["png_rho_masked"])


def test_reference_checkpoint_round_trip(tmp_path):
    """A Lightning checkpoint with the reference's 92 key names / shapes (golden) loads into Model and the
    canonical blob the kernels read follows; reference_checkpoint() writes the same names back."""
    from refnerf_pl_amd import configs, models, synthetic, utils
    g = np.load(os.path.join(ROOT, "tests", "golden", "io.npz"))
    configs.clear_config()
    configs.parse_config_files_and_bindings([GIN], [])
    model = models.construct_model(utils.dummy_rays(), configs.Config())
    blob = synthetic.make_params(seed=11, bias_scale=0.05)
    sd = {}
    for key, shp in zip(g["ckpt_keys"], g["ckpt_shapes"]):
        name = str(key)[len("model."):].split(".", 1)[1]                 # strip model.<nerf|prop>_mlp.
        spec = next(s for s in layout.PARAM_SPECS if name in (s.name + ".weight", s.name + ".bias"))
        shape = tuple(int(x) for x in str(shp).split(";"))
        if name.endswith(".weight"):
            t = blob[spec.w_off:spec.w_off + spec.out_dim * spec.in_dim].reshape(spec.out_dim, spec.in_dim)
        else:
            t = blob[spec.b_off:spec.b_off + spec.out_dim]
        assert t.shape == shape, key
        sd[str(key)] = torch.tensor(t)
    path = tmp_path / "last.ckpt"
    torch.save({"state_dict": sd, "epoch": 3, "global_step": 1234}, path)
    missing, unexpected = utils.load_reference_checkpoint(model, str(path))
    assert missing == [] and unexpected == []
    assert np.array_equal(model.nerf_mlp.flat_params().numpy(), blob)
    assert model.prop_mlp is model.nerf_mlp
    back = utils.reference_checkpoint(model, global_step=1234)
    assert sorted(back["state_dict"]) == sorted(str(k) for k in g["ckpt_keys"])
    for k, v in back["state_dict"].items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        utils.load_reference_checkpoint(model, {"state_dict": {"model.nerf_mlp.nope.weight": torch.zeros(1)}})


def test_train_ray_batcher_sampling_logic():
    """datasets.TrainRayBatcher (mirror of Dataset._next_train / _make_ray_batch, datasets.py:395-485) on CPU tensors,
    without casting rays: patch structure, pixel ranges, colour gather, per-rank streams, single-image batching."""
    from refnerf_pl_amd import camera_utils, datasets
    rng = np.random.default_rng(0)
    imgs = rng.random((4, 20, 30, 3)).astype(np.float32)
    p2c = np.tile(camera_utils.get_pixtocam(40.0, 30, 20)[None], (4, 1, 1))
    c2w = np.tile(np.eye(4, dtype=np.float32)[:3][None], (4, 1, 1))

    def make(**kw):
        return datasets.TrainRayBatcher(imgs, (p2c, c2w, None, None), 2., 6., 64, device="cpu", **kw)
    b = make(patch_size=2, seed=1)
    batch = b.next(cast_rays=False)
    px, py, cam = batch.rays.pix_x_int, batch.rays.pix_y_int, batch.rays.cam_idx[..., 0]
    assert px.shape == (16, 2, 2) and batch.rgb.shape == (16, 2, 2, 3)
    assert int(px.min()) >= 0 and int(px.max()) <= 29 and int(py.min()) >= 0 and int(py.max()) <= 19
    assert (px[:, :, 1] - px[:, :, 0] == 1).all() and (py[:, 1, :] - py[:, 0, :] == 1).all()      # patches are contiguous pixels
    assert (cam[:, 0, 0][:, None, None] == cam).all() and len(cam.unique()) > 1                      # one camera per patch
    assert np.array_equal(batch.rgb.numpy(), imgs[cam.numpy(), py.numpy(), px.numpy()])
    assert float(batch.rays.near.min()) == 2. and float(batch.rays.far.max()) == 6. and float(batch.rays.lossmult.min()) == 1.
    # same seed -> same stream; another rank -> another stream (the reference's ranks share one numpy stream: quirk B17)
    assert torch.equal(make(patch_size=2, seed=1).next(cast_rays=False).rays.pix_x_int, px)
    assert not torch.equal(make(patch_size=2, seed=1, rank=1).next(cast_rays=False).rays.pix_x_int, px)
    # single_image batching: one camera for the whole batch; debug mode: raster order from pixel (0, 0) of camera 0
    s = make(batching="single_image", seed=3).next(cast_rays=False)
    assert len(s.rays.cam_idx.unique()) == 1 and s.rays.pix_x_int.shape == (64, 1, 1)
    d = make(debug_mode=True).next(cast_rays=False)
    assert d.rays.pix_x_int.reshape(-1)[:3].tolist() == [0, 1, 2] and int(d.rays.cam_idx.max()) == 0
    with pytest.raises(ValueError):
        make(batching="per_pixel")


def test_bench_compact_line_fits_the_driver_tail():
    """BENCH_r03.json had parsed = null because bench.py's one JSON line (20.6 KB) overflowed the ~8 KB
    stdout tail the driver parses.  The LAST stdout line is now `bench.compact_line(full)`: <= 4 KB, with the contract's
    keys, `roofline` and `cpu_baseline`; the full record goes to gpurun_out/bench_full.json + stderr.  Replayed here on the
    full records of round 3 (the largest ones this repo ever printed)."""
    import glob
    import json
    import bench
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r03", "bench", "*.json")) + glob.glob(os.path.join(ROOT, "profiles", "r04", "bench", "*.full.json"))
                   + glob.glob(os.path.join(ROOT, "profiles", "r05", "bench", "*.full.json")))
    assert paths and any("r05" in p for p in paths)
    for p in paths:
        full = json.load(open(p))
        # (round 3's C5 record predates the training configuration's cpu_baseline leg)
        full.setdefault("cpu_baseline", {"value": 1.0e5, "unit": "ray-samples/s", "cores": 256, "kind": "port", "sample": "x" * 200})
        line = bench.compact_line(full)
        text = json.dumps(line)
        assert len(text) < bench.COMPACT_LIMIT <= 4096, (p, len(text))
        assert "\n" not in text
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config", "roofline", "cpu_baseline"):
            assert k in line, (p, k)
        assert "workload" in line["config"] and "model" not in line["config"]
        for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert k in line["roofline"], (p, k)
        assert abs(line["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-4
        if os.sep + "r05" + os.sep in p and os.path.basename(p).startswith("bench_C2"):   # (the PMC passes are collected at C2)
            # what the kernel is actually bound by travels with the number -- the matrix pipe's busy fraction,
            # the flops it executes as a fraction of the dense f16 peak, and the clock it sustained (profiles/traffic.json)
            for k in ("mfma_busy", "executed_flop_frac", "sustained_clock_ghz"):
                assert isinstance(line["roofline"].get(k), float) and 0 < line["roofline"][k] < 3, (p, k)
            assert line["roofline"]["traffic"] is not None
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in line["cpu_baseline"], (p, k)
        assert abs(line["value"] / full["value"] - 1) < 1e-4
        if "parity" in full:         # eval configurations: the oracle checks the timed batch
            assert "index_contract" in line["parity"] and line["parity"]["bench_batch"]["rgb_linf"] is not None
    # a pathological record (every optional block ten times its size) still fits: blocks are dropped, never the contract
    full = json.load(open(paths[0]))
    full["other_configs"] = {f"X{i}": v for i in range(10) for v in full["other_configs"].values()}
    for i in range(40):
        full[f"train_step_m{i}"] = full["train_step"]
    line = bench.compact_line(full)
    assert len(json.dumps(line)) < bench.COMPACT_LIMIT and "roofline" in line and "cpu_baseline" in line


def test_bench_stdout_carries_exactly_one_line(tmp_path):
    """RCCL prints its version banner on stdout through C stdio, flushed at exit -- after bench.py's JSON line (seen on the
    GPU box in round 4: the driver would have parsed "Librccl path : ..." as the last line).  bench.claim_stdout() points fd 1
    at stderr for everyone else; only emit()'s compact line reaches the real stdout."""
    import json
    import subprocess
    import sys
    rec = os.path.join(ROOT, "profiles", "r03", "bench", "bench_C2.json")
    code = (
        "import ctypes, json, os, sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import bench\n"
        "bench.ROOT = sys.argv[2]\n"                                   # (the full record's file goes to the temp dir)
        "bench.claim_stdout()\n"
        "print('python-level noise')\n"
        "os.write(1, b'fd-level noise\\n')\n"
        "libc = ctypes.CDLL(None)\n"
        "libc.printf(b'C stdio noise, flushed at exit\\n')\n"          # what RCCL's banner does
        "bench.emit(json.load(open(sys.argv[1])))\n")
    r = subprocess.run([sys.executable, "-c", code, rec, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert "roofline" in line and "cpu_baseline" in line and len(lines[0]) < 4096
    assert "python-level noise" in r.stderr and "fd-level noise" in r.stderr and "C stdio noise" in r.stderr
    assert "BENCH_FULL " in r.stderr and os.path.exists(tmp_path / "gpurun_out" / "bench_full.json")


def test_bench_plain_line_and_dump_outputs(tmp_path, monkeypatch, capsys):
    """A plain bench run prints the compact line alone (no full record named), and --dump-outputs writes the last step's
    arrays as float32 / float64 .npy files within the byte limit: whole when they fit, else every per-ray array on the same
    fixed, seeded ray sample (ray_index.npy), identical from run to run."""
    import json
    import sys
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "2", "--full", "--dump-outputs", str(tmp_path)])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and a.full and a.dump_outputs == str(tmp_path)
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert not bench.parse().full and bench.parse().dump_outputs is None
    bench.emit_line({"metric": "m", "value": 1.5e8, "unit": "ray-samples/s", "n_gpus": 1, "steps": 7, "warmup": 2, "ms_per_step": 2.5,
                     "higher_is_better": True, "dtype": "f16x2", "config": {"name": "C2"}})
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 1 and "full_record" not in json.loads(out[0])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(json.loads(out[0]))

    R, N = 64, 8
    g = torch.Generator().manual_seed(3)
    rend = [{"rgb": torch.rand(R, 3, generator=g), "acc": torch.rand(R, generator=g, dtype=torch.float64),
             "ray_sdist": torch.rand(4, N + 1, generator=g)} for _ in range(2)]
    hist = [{"rgb": torch.rand(R, N, 3, generator=g).bfloat16(), "weights": torch.rand(R, N, generator=g), "tint": None} for _ in range(2)]
    arrays = bench.eval_outputs((rend, hist))
    assert "level1_history_tint" not in arrays and "level0_rendering_ray_sdist" in arrays
    whole = bench.dump_outputs(str(tmp_path / "whole"), arrays, R)
    assert "ray_index" not in whole
    for k in whole:
        a = np.load(tmp_path / "whole" / (k + ".npy"))
        assert a.dtype == (np.float64 if k.endswith("_acc") else np.float32) and a.shape == tuple(arrays[k].shape), k
    monkeypatch.setattr(bench, "DUMP_BYTES", 8000)
    runs = [bench.dump_outputs(str(tmp_path / f"s{i}"), arrays, R) for i in range(2)]
    assert runs[0] == runs[1] and "ray_index" in runs[0]
    idx = np.load(tmp_path / "s0" / "ray_index.npy")
    assert 0 < idx.size < R and np.all(np.diff(idx) > 0) and np.array_equal(idx, np.load(tmp_path / "s1" / "ray_index.npy"))
    assert sum(np.load(tmp_path / "s0" / (k + ".npy")).nbytes for k in runs[0]) <= 8000
    w = np.load(tmp_path / "s0" / "level1_history_weights.npy")
    assert np.array_equal(w, arrays["level1_history_weights"].numpy()[idx.astype(np.int64)])
    assert np.load(tmp_path / "s0" / "level0_rendering_ray_sdist.npy").shape == (4, N + 1)


def test_data_loss_statistics_match_the_reference():
    """`Config.compute_normal_metrics` / `compute_disp_metrics`: the statistics branch of train_utils.compute_data_loss
    (internal/train_utils.py:62-84; VERDICT r4 missing 5) against the reference's own values on seeded renderings
    (tests/golden/normal_metrics.npz): weighted mean angular error of the normals in degrees per level, NaN when the
    renderings carry no normals (eval mode), disparity MSE, and the loss itself."""
    from refnerf_pl_amd import train_utils, utils
    g = np.load(os.path.join(ROOT, "tests", "golden", "normal_metrics.npz"))
    configs.clear_config()
    configs.parse_config_files_and_bindings([os.path.join(ROOT, "configs", "refnerf_blender.gin")],
                                            ["Config.compute_normal_metrics = True", "Config.compute_disp_metrics = True"])
    c = configs.Config()
    rays = utils.rays_from_dict({k[5:]: g[k] for k in g.files if k.startswith("rays_")}, torch.device("cpu"))
    for tag in ("train", "eval"):
        rend = [{k: torch.tensor(g[f"{tag}_L{lvl}_{k}"]) for k in ("rgb", "acc", "distance_mean", "normals") if f"{tag}_L{lvl}_{k}" in g.files}
                for lvl in range(2)]
        batch = utils.Batch(rays=rays, rgb=g[tag + "_gt_rgb"], disps=g[tag + "_disps"], normals=g[tag + "_normals"], alphas=g[tag + "_alphas"])
        loss, stats = train_utils.compute_data_loss(batch, rend, rays, c)
        assert float(loss) == pytest.approx(float(g[tag + "_loss"]), rel=1e-6)
        assert sorted(stats) == sorted(k[len(tag) + 6:] for k in g.files if k.startswith(tag + "_stat_"))
        for k, v in stats.items():
            np.testing.assert_allclose(v.numpy(), g[f"{tag}_stat_{k}"], rtol=2e-6, atol=0, equal_nan=True, err_msg=f"{tag} {k}")
    assert np.isnan(g["eval_stat_normal_maes"]).all() and np.isfinite(g["train_stat_normal_maes"]).all()
    configs.clear_config()


def test_non_finite_loss_guard_is_loud_one_step_later():
    """the 16-bit chain modes turn operands beyond 65504 into NaN outputs; train_utils.compute_losses watches every
    total (Config.hip_check_finite, default on) and raises FloatingPointError naming the knobs that lift the limit.  On the
    CPU the check is immediate; on a device the flag of step k is read when step k + 1 asks (no synchronisation)."""
    import torch
    from refnerf_pl_amd import configs, train_utils
    cfg = configs.Config()
    assert cfg.hip_check_finite is True
    guard = train_utils._FiniteGuard()
    guard.watch(torch.tensor(1.0), cfg)
    with pytest.raises(FloatingPointError, match="hip_train_precision"):
        guard.watch(torch.tensor(float("nan")), cfg)
    guard.watch(torch.tensor(2.0), cfg)          # usable afterwards
    train_utils.flush_finite_check(cfg)          # nothing pending on the module's own guard: no-op


def test_level_image_rule_lives_in_the_library():
    """ABI v11: which weight image a level configuration streams is ONE rule inside the library
    (refnerf_level_image; _hip.level_image only forwards to it) -- a pure host function, checked here without a GPU."""
    import ctypes as C
    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip
    assert _hip.lib().refnerf_level_image(None) == -1
    F32, BF16, F16, F16X2 = _hip.PREC_F32, _hip.PREC_BF16, _hip.PREC_F16, _hip.PREC_F16X2
    for prec in (F32, BF16, F16, F16X2):
        assert _hip.level_image(prec, False) == prec                     # inference: the image of the mode
        assert _hip.level_image(prec, False, 7) == F32                   # a general IPE basis: the (extended) f32 image
    assert _hip.level_image(F32, True) == F32 and _hip.level_image(BF16, True) == F32      # the f32 image carries the bf16 chain ops
    assert _hip.level_image(F16X2, True) == (F32 if _hip.LEGACY_F16X2_TRAIN else _hip.IMAGE_F16X2_TRAIN)
    assert _hip.level_image(F16X2, True, 7) == F32


def test_every_roofline_names_its_profile():
    """every PMC-derived figure of a bench line is reproducible from THIS round's committed profiles --
    profiles/traffic.json holds entries of one round only, the per-kernel summary each entry was condensed from exists under
    profiles/<round>/, and bench.py's roofline helpers name that file (`traffic_source`, `pmc_source`) for the headline kernel, the
    C3 ring variant and the kernels of the training step."""
    import json
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prof = json.load(open(os.path.join(root, "profiles", "traffic.json")))
    rounds = {v["round"] for k, v in prof.items() if not k.startswith("_")}
    assert rounds == {"r06"}, rounds
    for key in prof:
        if key.startswith("_"):
            continue
        kernel, _, cfg = key.partition("@")
        f = os.path.join(root, "profiles", "r06", f"pmc_{kernel.split('::')[-1]}{'_' + cfg if cfg else ''}.csv")
        assert os.path.exists(f), f
    assert os.path.exists(os.path.join(root, "profiles", "r06", "kernel_stats.csv")) and os.path.exists(os.path.join(root, "profiles", "r06", "kernel_stats_C3.csv"))
    for kernel, cfg, rays, n in (("rn::level_fwd_f16x2", "C2", 4096, 128), ("rn::level_fwd_f16x2_ring", "C3", 8192, 192),
                                 ("rn::level_fwd_train_sq_h", "C2", 4096, 128), ("rn::level_bwd_sq", "C2", 4096, 128),
                                 ("rn::wgrad_sq256_kernel", "C2", 4096, 128)):
        r = bench.mfma_roofline("f16x2", kernel, 2.0, 1, 1e12, cfg, rays, n)
        assert r["traffic"] and "profiles/r06/pmc_" in r["traffic_source"], (kernel, r)
        assert "profiles/r06/pmc_" in r.get("pmc_source", ""), (kernel, r)
    line = bench.compact_line({"metric": "m", "value": 1.0, "dtype": "f16x2", "roofline": bench.mfma_roofline("f16x2", "rn::level_fwd_f16x2", 2.0, 1, 1e12, "C2", 4096, 128),
                               "timed_blocks": {"blocks": 5, "reported": "median", "ms_per_step": [1, 2, 3, 4, 5]}})
    assert line["roofline"]["pmc_source"].startswith("profiles/r06/pmc_level_fwd_f16x2.csv") and line["timed_blocks"]["blocks"] == 5


def test_scratch_of_the_training_kernels_is_what_design_md_states():
    """Code-object metadata of the built library (scripts/kernel_meta.py: private_segment_fixed_size = scratch bytes per lane,
    read with llvm-readelf -- no GPU needed): the backward of the mode of record and the weight-gradient GEMM hold every value
    in registers (round 5: 640 B/lane in the backward), the eval kernels of the three 16-bit modes likewise; the training
    forward of the mode of record likewise (round 5: 152 B/lane).  A build that regresses fails here, before any timing."""
    import importlib.util
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf on this host")
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(here, "scripts", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    meta = {k: v for k, v in km.kernel_meta(_hip.LIB_PATH).items()}

    def scratch(fragment):
        hits = [int(v["private_segment_fixed_size"]) for k, v in meta.items() if fragment in k]
        assert hits, fragment
        return max(hits)

    assert scratch("level_bwd_sq") == 0
    assert scratch("wgrad_sq256_kernel") == 0
    assert scratch("wgrad_sq_kernel") == 0
    for eval_kernel in ("level_fwd_f16x2ENS", "level_fwd_bf16ENS", "level_fwd_f16ENS",
                        "level_fwd_f16x2_ringENS", "level_fwd_bf16_ringENS", "level_fwd_f16_ringENS"):      # (ring variants: 16 B until round 6)
        assert scratch(eval_kernel) == 0, eval_kernel
    assert scratch("level_fwd_train_sq") == 0           # (both flavours; round 5: 152)


def test_wgrad_loops_hold_exactly_the_vector_memory_operations_their_waits_count(tmp_path):
    """The weight-gradient GEMM (refnerf_wgrad_sq.h, wgrad_sq256_raw_body) certifies the arrival of a k-step with
    `s_waitcnt vmcnt(VM * k)`: VM = the LDS-DMA instructions of one k-step and wave, counted in the source.  Any other vector-memory
    instruction the compiler put into those loops (a scratch reload, a re-fetched constant) would shift the count and let a wave read
    a ring slot before its data has landed.  This test compiles the translation unit to assembly (no GPU needed) and audits the four
    loop instances: exactly 5 (one-half jobs) / 7 (22-bit jobs) `global_load_lds_dwordx4`, nothing else from the vector-memory
    family, 16 / 32 MFMAs, and the one counted wait."""
    import shutil
    import subprocess
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this host")
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(here, "refnerf-pl_amd", "csrc")
    out = str(tmp_path / "sq_train.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-I" + os.path.join(here, "include"),
                           "-I" + csrc, "-S", "--cuda-device-only", os.path.join(csrc, "refnerf_sq_train.hip"), "-o", out], stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n")
    st = next(i for i, l in enumerate(lines) if re.match(r"_ZN2rn18wgrad_sq256_kernel\w*:", l))
    en = next(i for i in range(st, len(lines)) if ".amdhsa_kernel _ZN2rn18wgrad_sq256_kernel" in lines[i])
    loops = []
    for h in (i for i in range(st, en) if "Inner Loop Header" in lines[i]):
        label = lines[h].split(":")[0]
        back = [i for i in range(h, en) if re.search(r"s_c?branch\S*\s+" + re.escape(label) + r"\s*$", lines[i])]
        if back:
            loops.append([l.strip() for l in lines[h:back[-1] + 1] if l.strip() and not l.strip().startswith(";")])
    assert len(loops) == 4, len(loops)           # {bias wave, other wave} x {one-half jobs, 22-bit jobs}
    seen = set()
    for body in loops:
        vmem = [l.split()[0] for l in body if re.match(r"(global_|buffer_|scratch_|flat_)", l)]
        mfma = sum(1 for l in body if l.startswith("v_mfma"))
        waits = [l for l in body if "s_waitcnt" in l and "vmcnt" in l]
        assert set(vmem) == {"global_load_lds_dwordx4"}, vmem
        assert (mfma, len(vmem)) in ((16, 5), (32, 7)), (mfma, len(vmem))
        assert waits == (["s_waitcnt vmcnt(5)"] if mfma == 16 else ["s_waitcnt vmcnt(0)"]), waits
        seen.add(mfma)
    assert seen == {16, 32}
    shutil.rmtree(str(tmp_path), ignore_errors=True)
