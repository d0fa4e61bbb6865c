"""The LS-EEND front end without a GPU: the host plans (fluidaudio_amd/csrc/lseend_core.h through fa_lseend_plan_file / fa_lseend_plan_push)
against a literal restatement of the reference's two StreamingChunkQueues (LSEENDPreprocessor.swift:284-384) driven the way
LSEENDFeatureProvider drives them (:123-141 enqueue, :158-180 flush, :185-202 emit, :249-279 process), in samples and rows."""
import pytest

WIN, HOP, NFFT, MELS, CTX, SUB, DELAY = 200, 80, 256, 23, 7, 10, 9


class Queue:
    """StreamingChunkQueue counting elements instead of holding them"""

    def __init__(self, chunk, left, right):
        self.chunk, self.context, self.padded = chunk, left + right, chunk + left + right
        self.count, self.head = left, 0                       # seeded with `left` zeros

    unread = property(lambda self: self.count - self.head)

    def pop_next(self):
        if self.unread < self.padded:
            return None
        span = (self.head, self.head + self.padded)
        self.head += self.chunk
        return span

    def pop_all(self):
        if self.unread < self.padded:
            return None
        new_head = self.head + (self.count - self.head - self.context) // self.chunk * self.chunk
        span = (self.head, new_head + self.context)
        self.head = new_head
        return span


class Provider:
    """LSEENDFeatureProvider's bookkeeping; one call = enqueue (and drain), then emitNextChunk until it gives nil"""

    def __init__(self, chunk):
        self.chunk = chunk
        self.audio = Queue(HOP * SUB * chunk, NFFT // 2, NFFT // 2 - HOP)
        self.mel = Queue(SUB * chunk, CTX, CTX + 1 - SUB)
        self.flush_samples = (CTX + DELAY * SUB) * HOP + NFFT // 2
        self.mask = [0.0] * DELAY + [1.0] * chunk
        self.mask_end = self.frames = 0

    def process(self):
        span = self.audio.pop_all()
        if span:
            frames = max(0, (span[1] - span[0] - NFFT) // HOP + 1)     # .prePadded
            self.mel.count += frames
            self.frames += frames

    def call(self, samples, flush):
        before = self.frames
        self.audio.count += samples
        self.process()
        if flush:
            self.audio.count += self.flush_samples
            over = max(0, self.audio.unread - self.audio.context)
            self.audio.count += (self.audio.chunk - over % self.audio.chunk) % self.audio.chunk
            self.process()
        warmups, masks, starts = [], [], []
        while True:
            span = self.mel.pop_next()
            if not span:
                break
            self.mask_end = min(self.mask_end + self.chunk, len(self.mask))
            masks.append(self.mask[self.mask_end - self.chunk:self.mask_end])
            warmups.append(min(len(self.mask) - self.mask_end, self.chunk))
            starts.append(span[0])
        return dict(frames=self.frames - before, warmups=warmups, masks=masks, starts=starts, unread_audio=self.audio.unread, unread_mel=self.mel.unread,
                    mask_end=self.mask_end)


def agree(plan, warmups, masks, want, chunk):
    assert (plan.frames, plan.windows, plan.unread_audio, plan.unread_mel_rows, plan.decoder_mask_end) == \
        (want["frames"], len(want["warmups"]), want["unread_audio"], want["unread_mel"], want["mask_end"])
    assert warmups.tolist() == want["warmups"] and masks.tolist() == want["masks"]
    assert [plan.stream_window0 + k for k in range(plan.windows)] == [s // (SUB * chunk) for s in want["starts"]]
    assert plan.out_rows == sum(chunk - w for w in want["warmups"])


@pytest.mark.parametrize("chunk", [1, 5])
def test_file_plan_equals_the_queues(fa, chunk):
    cfg = fa.lseend_config(chunk_size=chunk)
    assert fa.lseend_mel_frames(cfg) == (chunk - 1) * SUB + 2 * CTX + 1
    one = HOP * SUB * chunk
    lengths = [0, 1, one - 1, one, one + 1, 3 * one + 4321]
    plans, warmups, masks = fa.lseend_plan_file(lengths, cfg)
    at = rows = frames = 0
    for n, plan in zip(lengths, plans):
        want = Provider(chunk).call(n, True)
        assert (plan.window0, plan.out_row0, plan.frame0) == (at, rows, frames) and len(want["warmups"]) > 0
        agree(plan, warmups[at:at + plan.windows], masks[at:at + plan.windows], want, chunk)
        at, rows, frames = at + plan.windows, rows + plan.out_rows, frames + plan.frames
    assert at == len(warmups)


@pytest.mark.parametrize("chunk", [1, 5])
def test_pushes_in_pieces_equal_the_queues_and_end_where_the_file_plan_ends(fa, chunk):
    cfg = fa.lseend_config(chunk_size=chunk)
    pieces = [1, 79, 800, 4001] * 3
    ref, state = Provider(chunk), fa._lib.LseendStreamInfo()
    frames = windows = rows = 0
    for i, n in enumerate(pieces + [0]):
        flush = i == len(pieces)
        plan, warmups, masks = fa.lseend_plan_push(state, n, flush, cfg)
        agree(plan, warmups, masks, ref.call(n, flush), chunk)
        assert (state.frames, state.windows, state.unread_audio, state.unread_mel_rows) == (frames + plan.frames, windows + plan.windows, plan.unread_audio, plan.unread_mel_rows)
        frames, windows, rows = frames + plan.frames, windows + plan.windows, rows + plan.out_rows
    whole = fa.lseend_plan_file([sum(pieces)], cfg)[0][0]
    assert (whole.frames, whole.windows, whole.out_rows, whole.unread_audio, whole.unread_mel_rows) == (frames, windows, rows, state.unread_audio, state.unread_mel_rows)


def test_status_contract_needs_no_gpu(fa):
    lib = fa.lib()
    assert lib.fa_lseend_mel_frames(None) == 0
    for bad in (dict(n_fft=512, win=400), dict(hop=129), dict(subsampling=16), dict(n_mels=129)):
        cfg = fa.lseend_config(**bad)
        # n_fft 512 is a sound geometry that this kernel generation refuses when it builds its tables; the others are no geometry at all
        assert (fa.lseend_mel_frames(cfg) == 0) == ("n_fft" not in bad)
