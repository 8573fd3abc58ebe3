"""CPU: the decoding rule's restatement (tests/decode_ref.py) checked on its own - Philox known answers, the uniform's
range, the distribution it draws - and the Trainer's generation surface on an engine without rollout(): defaults, knobs,
and the refusal to sample where no decode kernel exists."""
import numpy as np
import pytest
import torch

import decode_ref as D
from helpers import oracle_factory, reference_args
from oracle import layout_spec as O

SMALL = dict(batch_size=4, epochs=1, print_freq=1, n_frames=4, n_slots=8, d_model=64, n_layers=1, train_clips=8, val_clips=4)


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    src = tmp_path / "src"
    src.mkdir()
    monkeypatch.chdir(src)
    for k in ("VLG_MODEL", "VLG_GEN_TEMPERATURE", "VLG_GEN_TOP_K", "VLG_GEN_SEED", "VLG_GEN_KEEP_PADDED"):
        monkeypatch.delenv(k, raising=False)
    return tmp_path


def _words(w):
    return " ".join("%08x" % int(x) for x in w)


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10"""
    assert _words(D.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _words(D.philox4x32_10((ones,) * 4, (ones,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _words(D.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over the counter = the scalar evaluation, element by element
    tok = np.array([0, 1, 77, 2 ** 31 - 1])
    z = np.zeros_like(tok)
    vec = D.philox4x32_10((tok, z + 3, z, z), (z + 5, z + 9))
    for i, t in enumerate(tok):
        assert [int(w[i]) for w in vec] == [int(w) for w in D.philox4x32_10((int(t), 3, 0, 0), (5, 9))]


def test_uniform_is_strictly_inside_the_unit_interval():
    u = D.uniform(np.arange(1 << 16), 3, 0x123456789ABCDEF)
    assert u.dtype == np.float64 and float(u.min()) > 0.0 and float(u.max()) < 1.0
    # the extremes of the construction: x0 >> 8 = 0 and 2^24 - 1
    assert 0.0 * 2.0 ** -24 + 2.0 ** -25 > 0.0 and (2 ** 24 - 1) * 2.0 ** -24 + 2.0 ** -25 < 1.0
    assert abs(float(u.mean()) - 0.5) < 5 * (1 / 12 / u.size) ** 0.5
    # token, step and both halves of the seed all reach the draw
    base = D.uniform(np.arange(64), 0, 7)
    for other in (D.uniform(np.arange(64) + 64, 0, 7), D.uniform(np.arange(64), 1, 7), D.uniform(np.arange(64), 0, 8),
                  D.uniform(np.arange(64), 0, 7 + (1 << 32))):
        assert not np.array_equal(base, other)


def test_decode_step_edges():
    l = np.array([[0.0, 2.0, 2.0, -1.0], [5.0, 5.0, 5.0, 5.0]])
    assert D.decode_step(l, 0, 0.0, 0, 1)[0].tolist() == [1, 0]                      # first maximum
    for t in (0.5, 1.0, 4.0):
        assert D.decode_step(l, 0, t, 1, 1)[0].tolist() == [1, 0]                    # top-1 = argmax at any temperature
    draws = np.stack([D.decode_step(np.tile(l[:1], (512, 1)), s, 1.0, 2, 9)[0] for s in range(4)])
    assert set(draws.reshape(-1).tolist()) == {1, 2}                                 # ties: the LOWER indices are kept (1, 2; never 0, 3)
    cls, box, near = D.next_frame(torch.tensor([[0.0, 9.0, 0.0, 0.0, 0.0, 0.0]]), torch.tensor([[[2]]]), torch.rand(1, 1, 1, 4), 2, 0)
    assert cls.tolist() == [[1]] and torch.equal(box, torch.full((1, 1, 4), 0.5, dtype=torch.float64))


@pytest.mark.parametrize("temperature,top_k", D.DIST_CASES)
def test_restatement_draws_the_distribution(temperature, top_k):
    logits = np.tile(D.distribution_row().double().numpy(), (D.DIST_TOKENS, 1))
    classes = np.stack([D.decode_step(logits, s, temperature, top_k, D.DIST_SEED)[0] for s in range(D.DIST_STEPS)])
    D.check_distribution(classes, temperature, top_k)


def _host_loop(tr, cls, box, steps):
    """the rollout as the Trainer has always run it on such an engine: argmax, sigmoid, slide"""
    p = tr.engine.named_params()
    out_c, out_b = [], []
    with torch.no_grad():
        for _ in range(steps):
            logits, raw = O.forward(p, cls, box, tr.cfg.n_layers)
            nc, nb = logits[:, -1].argmax(-1), torch.sigmoid(raw[:, -1])
            out_c.append(nc)
            out_b.append(nb)
            cls, box = D.slide(cls, box, nc, nb)
    return torch.stack(out_c, 1), torch.stack(out_b, 1)


def test_trainer_default_generation_is_unchanged_and_sampling_is_refused(workdir):
    from trainer import Trainer
    tr = Trainer(reference_args(workdir / "exp", **SMALL), engine_factory=oracle_factory)
    assert not hasattr(tr.engine, "rollout")
    batch = next(iter(tr.val_loader))
    cls, box = batch["slot_class"], batch["slot_box"]
    want_c, want_b = _host_loop(tr, cls.clone(), box.clone(), 3)
    c, b = tr.generate_sequence(cls, box, steps=3)
    assert c.dtype == torch.int64 and b.dtype == torch.float32 and c.shape == (4, 3, 8) and b.shape == (4, 3, 8, 4)
    assert torch.equal(c, want_c) and torch.equal(b, want_b)
    c2, b2 = tr.generate_sequence(cls, box, steps=3, temperature=0.0, top_k=5, seed=3)   # argmax: top_k and seed are idle
    assert torch.equal(c2, c) and torch.equal(b2, b)
    with pytest.raises(ValueError, match="rollout"):
        tr.generate_sequence(cls, box, steps=3, temperature=0.8)
    with pytest.raises(ValueError, match="rollout"):
        tr.generate_sequence(cls, box, steps=3, keep_padded=True)


def test_generation_knobs_args_over_environment_over_default(workdir, monkeypatch):
    from trainer import Trainer, generation_knobs
    a = reference_args(workdir / "exp", **SMALL)
    assert generation_knobs(a) == {"temperature": 0.0, "top_k": 0, "seed": 1024, "keep_padded": False}
    assert generation_knobs(reference_args(workdir / "exp", seed=77, **SMALL))["seed"] == 77       # default seed = args.seed
    monkeypatch.setenv("VLG_GEN_TEMPERATURE", "0.7")
    monkeypatch.setenv("VLG_GEN_TOP_K", "5")
    monkeypatch.setenv("VLG_GEN_SEED", "12345678901")
    monkeypatch.setenv("VLG_GEN_KEEP_PADDED", "1")
    assert generation_knobs(a) == {"temperature": 0.7, "top_k": 5, "seed": 12345678901, "keep_padded": True}
    b = reference_args(workdir / "exp", gen_temperature=1.5, gen_top_k=3, gen_seed=9, gen_keep_padded=0, **SMALL)
    assert generation_knobs(b) == {"temperature": 1.5, "top_k": 3, "seed": 9, "keep_padded": False}
    # the environment's temperature reaches generate_sequence (refused on this engine); a keyword argument wins over it
    tr = Trainer(reference_args(workdir / "exp", **SMALL), engine_factory=oracle_factory)
    batch = next(iter(tr.val_loader))
    with pytest.raises(ValueError, match="rollout"):
        tr.generate_sequence(batch["slot_class"], batch["slot_box"], steps=1)
    c, _ = tr.generate_sequence(batch["slot_class"], batch["slot_box"], steps=1, temperature=0.0, keep_padded=False)
    assert c.shape == (4, 1, 8)
