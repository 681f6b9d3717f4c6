"""The image output path end to end on the tiny network of tests/test_generate_step_gpu.py (tests/golden/tiny_sampler.npz): image_grid,
to_uint8 and save_images against the restatement, SummarySink under make_log_sample, generate_to_dir at two batch sizes, a
"dataset"-mode round trip through the loader, and that writing moves no state."""
import os
import types

import numpy as np
import pytest
import torch

import image_out_cases as IO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_sampler.npz")
SIZE, STEPS = 16, 6
F32 = 0
TAGS = {"denoised", "step_1", "step_0.25", "step_0.5", "step_0.75", "fake", "epsilon_theta"}


def tiny(gpu, **kw):
    import gan_class_transfer2_amd as g
    z = np.load(GOLDEN)
    eng = g.UNetEngine(g.Topology(8, 16, 2), F32, gpu, steps=STEPS, **kw)
    eng.set_params({k[6:]: z[k] for k in z.files if k.startswith("param/")})
    return eng


def den(eng):
    return types.SimpleNamespace(ensure_engine=lambda: eng)


def decode(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.array(im)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def test_grid_conversion_and_png_equal_the_restatement(gpu, tmp_path):
    import gan_class_transfer2_amd as g
    imgs = IO.images_for((5, 6, 8))
    x = torch.from_numpy(imgs).to(gpu)
    for mode, code in IO.MODES.items():
        assert np.array_equal(host(g.to_uint8(x, mode)), IO.quantize_ref(imgs, code))
    assert np.array_equal(host(g.to_uint8(x)), IO.quantize_ref(imgs, IO.SUMMARY))
    grid = g.image_grid(x)                                  # cols = ceil(sqrt(5)) = 3, padding 2, black
    assert tuple(grid.shape) == g.grid_shape(5, 6, 8) + (3,) == (18, 32, 3) and grid.dtype == torch.uint8
    assert np.array_equal(host(grid), IO.grid_ref(imgs, IO.SUMMARY, 3, 2, 2, 1))
    kw = dict(cols=2, padding=1, scale=3, fill=IO.FILL, mode="dataset")
    assert np.array_equal(host(g.image_grid(x.to(torch.bfloat16), **kw)),
                          IO.grid_ref(x.to(torch.bfloat16).float().cpu().numpy(), IO.DATASET, 2, 3, 1, 3, IO.FILL))
    path = g.save_images(x, str(tmp_path / "sub" / "grid.png"), **kw)
    assert np.array_equal(decode(path), host(g.image_grid(x, **kw)))
    with pytest.raises(ValueError, match="mode"):
        g.to_uint8(x, "srgb")
    with pytest.raises(g.Gct2Error, match="scale=17"):
        g.image_grid(x, scale=17)


def test_writer_takes_device_tensors(gpu, tmp_path):
    import gan_class_transfer2_amd as g
    pics = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (7, 9, 5, 3), dtype=np.uint8)).to(gpu)
    with g.ImageWriter(str(tmp_path), threads=2, max_pending=2) as w:
        paths = w.write_many([f"m/{i}.png" for i in range(4)], pics[:4])
        paths += [w.write(f"s/{i}.png", pics[i]) for i in range(4, 7)]
    assert all(np.array_equal(decode(p), pics[i].cpu().numpy()) for i, p in enumerate(paths))


def test_summary_sink_under_make_log_sample(gpu, tmp_path):
    import gan_class_transfer2_amd as g
    z = np.load(GOLDEN)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
    eng = tiny(gpu)
    args = (t(z["example_image"]), t(z["example"]), t(z["dictionary"]))
    want = g.log_sample(den(eng), *args, steps=STEPS, test_step=2)
    assert {k for k, v in want.items() if v.dim() == 4} == TAGS == set(g.image_out.SUMMARY_TAGS)
    calls = []

    def log_sample(denoiser, *a, **kw):
        calls.append(1)
        return g.log_sample(denoiser, *a, steps=STEPS, test_step=2, **kw)

    logs = str(tmp_path / "logs")
    sink = g.SummarySink(logs, max_outputs=4, scale=2)
    sampler = g.sampler
    original, sampler.log_sample = sampler.log_sample, log_sample
    try:
        cb = g.make_log_sample(den(eng), *args, sink=sink)
        cb(0, None)
        cb(7, None)
    finally:
        sampler.log_sample = original
    assert len(calls) == 2 and sorted(os.listdir(logs)) == sorted(TAGS | {"scalars.csv"})
    for tag in TAGS:
        assert sorted(os.listdir(os.path.join(logs, tag))) == ["000000.png", "000007.png"]
        shown = want[tag][:4]
        k, q = shown.shape[0], host(g.to_uint8(shown))
        assert k == min(4, want[tag].shape[0])
        row = np.concatenate(list(q), axis=1)              # one row, no padding
        for name in ("000000.png", "000007.png"):
            assert np.array_equal(decode(os.path.join(logs, tag, name)), np.repeat(np.repeat(row, 2, 0), 2, 1)), (tag, name)
    rows = open(os.path.join(logs, "scalars.csv")).read().split()
    loss = float(want["example_loss"])
    assert rows[0] == "epochs,example_loss" and [r.split(",")[0] for r in rows[1:]] == ["0", "7"]
    assert all(np.float32(r.split(",")[1]) == np.float32(loss) for r in rows[1:])
    sink.close()


def test_generate_to_dir_does_not_depend_on_the_batch_size(gpu, tmp_path):
    import gan_class_transfer2_amd as g
    eng = tiny(gpu)
    kw = dict(num_steps=3, eta=0.7, seed=11, size=SIZE, clip_denoised=True)
    want = host(g.to_uint8(g.generate(den(eng), 5, **kw)))
    a = g.generate_to_dir(den(eng), 5, str(tmp_path / "a"), batch_size=2, **kw)
    b = g.generate_to_dir(den(eng), 5, str(tmp_path / "b"), batch_size=5, **kw)
    assert [os.path.basename(p) for p in a] == [f"{i:06d}.png" for i in range(5)] == sorted(os.listdir(tmp_path / "a"))
    assert sorted(os.listdir(tmp_path / "b")) == [os.path.basename(p) for p in b]
    for i in range(5):
        assert np.array_equal(decode(a[i]), want[i]) and np.array_equal(decode(b[i]), want[i]), i
    with g.ImageWriter(str(tmp_path), threads=1, max_pending=1) as w:
        c = g.generate_to_dir(den(eng), 2, str(tmp_path / "c"), pattern="s{:03d}.png", first_index=3, batch_size=1, writer=w, **kw)
    assert [os.path.basename(p) for p in c] == ["s003.png", "s004.png"]
    assert np.array_equal(decode(c[0]), want[3]) and np.array_equal(decode(c[1]), want[4])
    with pytest.raises(ValueError, match="return_steps"):
        g.generate_to_dir(den(eng), 2, str(tmp_path / "d"), return_steps=(6,), **kw)
    # Denoiser.generate_to_dir forwards
    from gan_class_transfer2_amd import model as M
    fake_self = den(eng)
    d = M.Denoiser.generate_to_dir(fake_self, 2, str(tmp_path / "e"), **kw)
    assert np.array_equal(decode(d[1]), want[1])


def test_dataset_mode_files_are_the_source_crops_byte_for_byte(gpu, tmp_path):
    import gan_class_transfer2_amd as g
    rng = np.random.default_rng(8)
    sources = [rng.integers(0, 256, (20, 24, 3), dtype=np.uint8) for _ in range(4)]
    ds = g.CachedImageDataset(sources, size=16, batch_size=4, device=gpu, seed=5)
    picks = torch.zeros(4, 4, dtype=torch.int32, device=gpu)
    batch = ds.batch_at(0, 4, picks_out=picks)
    with g.ImageWriter(str(tmp_path)) as w:
        paths = w.write_many([f"{i}.png" for i in range(4)], g.to_uint8(batch, "dataset"))
    for (item, oy, ox, flip), p in zip(host(picks).tolist(), paths):
        crop = sources[item][oy:oy + 16, ox:ox + 16]
        assert np.array_equal(decode(p), crop[:, ::-1] if flip else crop)
    # ... and the folder is a dataset again
    again = g.ImageDataset.validation(str(tmp_path / "*.png"), size=16, batch_size=4, device=gpu)
    x = next(iter(again))[0]
    assert np.array_equal(host(g.to_uint8(x, "dataset")), np.stack([decode(p) for p in sorted(paths)]))


def test_writing_moves_no_state(gpu, tmp_path):
    """generate and a train step after writing are bit-identical to the same calls on an engine that never wrote.  Both engines take one
    train step first (a recorded plan and optimizer slots exist), then the control takes the writer's parameters bit for bit: on this
    engine the Dense(3) bias `dense.b` is the one result of a train step that is not reproducible from run to run (measured: two
    engines built alike differ there by one float32 place after one step in about half the runs, in nothing else, and their losses
    agree), so without the copy the control would not be a control, and `dense.b` is the one parameter left out of the last
    comparison.  Every other parameter, the loss, the samples and the RNG positions must agree in every bit."""
    import gan_class_transfer2_amd as g
    x = torch.tensor(np.floor(np.random.default_rng(4).uniform(0, 256, (2, SIZE, SIZE, 3))) / 128 - 1, dtype=torch.float32, device=gpu)
    A, B = tiny(gpu, rng_seed=9), tiny(gpu, rng_seed=9)
    for eng in (A, B):
        eng.base_lr, eng.warm_up = 1e-2, 0
        eng.train_step(x)
    B.set_params(A.get_params())
    position = lambda eng: (eng.rng_offset_t, eng.rng_offset_eps, eng.iterations)
    same = lambda p, q: torch.equal(p.contiguous().view(torch.int32), q.contiguous().view(torch.int32))
    kw = dict(num_steps=3, eta=0.7, seed=2, size=SIZE)
    before, control = g.generate(den(A), 3, **kw).clone(), g.generate(den(B), 3, **kw).clone()
    torch.cuda.synchronize()
    assert same(before, control)                             # (the control is one: the two engines agree before anything is written)
    state = position(A)
    g.generate_to_dir(den(A), 3, str(tmp_path / "w"), batch_size=2, **kw)
    g.save_images(before, str(tmp_path / "grid.png"), scale=2)
    with g.ImageWriter(str(tmp_path)) as w:
        g.SummarySink(str(tmp_path / "logs"), writer=w)(0, {"fake": before, "example_loss": torch.ones(1, device=gpu)})
    assert position(A) == state == position(B)
    after, never = g.generate(den(A), 3, **kw), g.generate(den(B), 3, **kw)
    la, lb = A.train_step(x).clone(), B.train_step(x).clone()
    torch.cuda.synchronize()
    assert same(before, after) and same(after, never) and same(la, lb)
    assert position(A) == position(B) != state
    pa, pb = A.get_params(), B.get_params()
    assert set(pa) == set(pb) and "dense.b" in pa
    differ = [k for k in pa if k != "dense.b" and not np.array_equal(pa[k].view(np.int32), pb[k].view(np.int32))]
    assert not differ, differ
