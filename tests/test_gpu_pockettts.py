"""The PocketTTS session on the device (fluidaudio_amd/csrc/pockettts.hip) against the numpy restatement of the reference's host code
(tests/pockettts_restatement.py).  Everything is compared for equality except the re-projection of Gaussian inputs, whose bound is
max|device - float64| <= 4 max|float32 numpy emulation - float64|, both printed."""
import functools

import numpy as np
import pytest

import pockettts_restatement as R

pytestmark = pytest.mark.gpu

POISON = np.float32(-7.25e30)


@functools.lru_cache(None)
def small(fa, gpu_ctx, bos_sequence):
    """one layer, five streams, a cache of one position: the re-projection, prefill and step tests need no large cache"""
    return fa.PocketTtsSession(fa.pockettts_config(layers=1, streams=5, voices=4, voice_seq=1, projections=2, vocab=7, windows=8, clones=3, max_frames=16,
                                                   bos_sequence=bos_sequence), gpu_ctx)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    nan = np.isnan(a)
    return a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(u)[~nan], b.view(u)[~nan])


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("frames", [1, 31, 32, 33, 125])
def test_reprojection(fa, gpu_ctx, frames, dtype, strided):
    s, rng = small(fa, gpu_ctx, 0), np.random.default_rng(frames)
    fs, ds = (1040, 2) if strided else (1024, 1)
    item = 125 * fs + 2048
    for gaussian in (False, True):
        draw = (lambda shape, scale: rng.standard_normal(shape) / scale) if gaussian else (lambda shape, scale: rng.integers(-4, 5, shape))
        projs = [(draw((1024, 32), 32).astype(np.float32), draw((1024, 32), 6).astype(np.float32)) for _ in range(2)]
        for i, (p, w) in enumerate(projs):
            s.set_projection(i, p, w)
        flat = draw(3 * item, 1).astype(dtype)
        cond = np.lib.stride_tricks.as_strided(flat, (3, frames, 1024), tuple(x * flat.itemsize for x in (item, fs, ds)))
        s.put("voice_rows", np.full(3 * 125 * 1024, POISON))
        s.clone([0, 1, 2], [0, 1, -1], frames, cond)
        for b, proj in enumerate([0, 1, -1]):
            rows, got = R.extract(flat[b * item:], frames, fs, ds), s.voice_rows(b)
            assert np.all(got[frames:] == POISON), "rows at or past usable were written"
            if proj < 0:
                assert same_bits(got[:frames], rows)
                continue
            pinv, w = projs[proj]
            want = R.reproject(rows, pinv, w)
            if not gaussian:
                assert np.array_equal(got[:frames].astype(np.float64), want), np.argwhere(got[:frames] != want)[:4]
                continue
            err, emu = np.abs(got[:frames] - want).max(), np.abs(R.reproject(rows, pinv, w, np.float32) - want).max()
            print(f"reprojection frames {frames} {np.dtype(dtype).name} strided {strided}: device {err:.3e}, float32 emulation {emu:.3e}")
            assert err <= 4 * emu


SPECIAL = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 1e-7, 6.1e-5, 65519.9, 65520.0, 1e6, -1e6,
                    0.0, -0.0, np.nan, np.inf, -np.inf, -(1 + 2.0 ** -11)], np.float32)


@pytest.mark.parametrize("kv_format", [0, 1, 2])
@pytest.mark.parametrize("src_seq", [0, 1, 125, 512])
def test_kv_reset(fa, gpu_ctx, src_seq, kv_format):
    s = fa.PocketTtsSession(fa.pockettts_config(layers=2, kv_format=kv_format, streams=3, voices=3, voice_seq=512, projections=0, vocab=1, windows=1, clones=1, max_frames=1), gpu_ctx)
    rng = np.random.default_rng(src_seq)
    voices = [[rng.standard_normal(2 * src_seq * 1024).astype(np.float32) * 40 for _ in range(2)] for _ in range(2)]
    if src_seq:
        voices[0][0][:SPECIAL.size] = SPECIAL
        voices[0][1][-SPECIAL.size:] = SPECIAL
    offsets = [[src_seq, src_seq + 1], [7, 9]]
    assert s.add_voice(0, voices[0], offsets[0], src_seq) == 0 and s.add_voice(1, voices[1], offsets[1], src_seq) == 0
    assert s.add_voice(2, voices[0][:1], [0], src_seq) == 2 and s.add_voice(2, voices[0], offsets[0], 513) == 3
    assert s.add_voice(2, [voices[0][0], voices[0][1][1:]], offsets[0], src_seq) == (4 if src_seq else 0)
    s.clone([2], [-1], [0], np.zeros((1, 1, 1024), np.float32))            # voice 2: cloned, no snapshot
    slab = np.full(3 * 2 * 2 * 512 * 1024, np.nan, np.float16 if kv_format == 2 else np.float32)
    s.put("kv", slab)
    s.put("positions", np.full(3 * s.n_positions, np.nan, np.float32))
    s.kv_reset([2, 0, 1], [1, 0, 2])                                        # stream 2 <- voice 1, stream 0 <- voice 0, stream 1 <- the cloned voice

    def check(stream, layers, offs):
        want, pos = R.kv_from_snapshot(layers, offs, src_seq, kv_format)
        assert np.array_equal(s.positions()[stream], pos)
        for layer in range(2):
            for side in range(2):
                got = s.kv_plane(stream, layer, side)
                assert same_bits(got, want[layer][side] if want else np.zeros_like(got)), (stream, layer, side)
    check(0, voices[0], offsets[0])
    check(2, voices[1], offsets[1])
    check(1, None, [0, 0])
    before = [s.kv_plane(0, layer, side) for layer in range(2) for side in range(2)]
    s.kv_capture(0, 2, 512)                                                 # the whole of stream 0 becomes voice 2's snapshot
    s.put("kv", slab)
    s.kv_reset([1], [2])
    assert all(same_bits(s.kv_plane(1, layer, side), before[2 * layer + side]) for layer in range(2) for side in range(2))
    assert np.array_equal(s.positions()[1], np.float32(offsets[0][:s.n_positions]))
    s.close()


@pytest.mark.parametrize("have_bos", [True, False])
@pytest.mark.parametrize("voice_frames", [0, 125])
@pytest.mark.parametrize("tokens", [0, 1, 255, 256, 257])
def test_prefill_inputs(fa, gpu_ctx, tokens, voice_frames, have_bos):
    s, rng = small(fa, gpu_ctx, 0), np.random.default_rng(tokens)
    table, bos = rng.standard_normal((7, 1024)).astype(np.float32), rng.standard_normal(1024).astype(np.float32)
    s.set_constants(table, bos if have_bos else None)
    rows = rng.standard_normal((1, 125, 1024)).astype(np.float32)
    s.clone([0], [-1], [voice_frames], rows)
    assert s.add_voice(1, [np.zeros(0, np.float32)], [0], 0) == 0          # a shipped voice: no voice block
    ids = [rng.integers(-1, 8, n).astype(np.int32) for n in (tokens, 300)]
    for a in ids:
        a[:1], a[-1:] = -1, 7
    s.set_position(3, 5.0)
    s.set_position(1, 40.0)
    s.put("windows", np.full(8 * 256 * 1024, np.nan, np.float32))
    wins, status = s.plan([3, 1], [0, 1], [tokens, 300])
    s.prefill_inputs(ids)
    want, wstat, rows_of = [], [], {}
    for stream, voice, tok, start in ((3, {"snapshot": False, "rows": rows[0, :voice_frames]}, ids[0], 5.0), (1, {"snapshot": True, "rows": None}, ids[1], 40.0)):
        st, blocks = R.prefill_blocks(voice, tok, table, bos if have_bos else None)
        wstat.append(st)
        before = 0
        for block, first, n, cond, valid in blocks:
            want.append((stream, block, first, n, cond, valid, np.float32(start + before)))
            before += n
        rows_of[stream] = np.float32(start + before)
    assert status.tolist() == wstat and len(wins) == len(want)
    arena = s.get("windows", 0, len(want) * 256 * 1024).reshape(len(want), 256, 1024)
    for i, (w, (stream, block, first, n, cond, valid, pos)) in enumerate(zip(wins, want)):
        assert (w.stream, w.block, w.first, w.n) == (stream, block, first, n)
        assert same_bits(arena[i], cond) and s.get("valid_len", i)[0] == valid and s.get("window_position", i)[0] == pos
    assert s.positions()[3, 0] == rows_of[3] and s.positions()[1, 0] == rows_of[1]


@pytest.mark.parametrize("bos_sequence", [0, 1])
@pytest.mark.parametrize("after", [0, 3])
def test_step(fa, gpu_ctx, after, bos_sequence):
    s, rng = small(fa, gpu_ctx, bos_sequence), np.random.default_rng(after)
    bos = rng.standard_normal(32).astype(np.float32)
    s.set_constants(np.zeros((1, 1024), np.float32), None, bos)
    max_gen = [7, 12, 9, 5]
    scripts = np.full((4, 13), -9.0, np.float32)
    scripts[1, 0], scripts[2, 8], scripts[3, :] = -3.5, 0.0, -4.0      # above at step 0; above at max_gen - 1; exactly the threshold: not EOS
    scripts[0, 3] = np.nan
    want = [R.generation_loop(scripts[i], max_gen[i], after) for i in range(4)]
    for i in range(5):
        s.set_position(i, 10.0 * i)
    assert s.step_begin([0, 1, 2, 3, 4], max_gen + [17], after).tolist() == [0, 0, 0, 0, 8]     # stream 4: more frames than its slab holds
    assert s.running().tolist() == [0, 1, 2, 3]
    seq = np.tile(bos if bos_sequence else np.full(32, np.nan, np.float32), (5, 1))
    assert same_bits(s.get("sequence", 0, 4 * 32), seq[:4].reshape(-1))
    latents, samples = rng.standard_normal((13, 5, 32)).astype(np.float32), rng.standard_normal((13, 5, 1920)).astype(np.float32)
    for t in range(13):
        s.step(np.append(scripts[:, t], np.float32(5.0)), latents[t])
        s.append_audio(samples[t])
        st = s.state()
        for i, (emitted, reason, calls) in enumerate(want):
            emit = t in emitted and t < calls
            if emit:
                seq[i] = latents[t, i]
            frames = sum(1 for e in emitted if e <= t)
            assert (st["emit"][i], st["frames"][i], st["reason"][i]) == (int(emit), frames, 1 if t + 1 < calls else reason), (t, i)
            assert s.positions()[i, 0] == np.float32(10.0 * i + frames)
        assert st["reason"][4] == 0 and s.running().tolist() == [i for i in range(4) if t + 1 < want[i][2]]
        assert same_bits(s.get("sequence", 0, 4 * 32), seq[:4].reshape(-1))
    assert [st["eos_step"][i] for i in range(4)] == [-1, 0, 8, -1]
    for i, (emitted, _, _) in enumerate(want):
        assert np.array_equal(s.audio(i, len(emitted)), samples[emitted, i])
