"""Host-side mirror of the TDT decoder's navigation helpers and greedy control loop (reference:
Sources/FluidAudio/ASR/Parakeet/SlidingWindow/TDT/Decoder/: TdtFrameNavigation.swift:20-105, TdtDurationMapping.swift:17-31,
TdtConfig.swift:13-26, TdtDecoderV3.swift:103-607) over the HIP C ABI (csrc/tdt.hip), and of its language mode (Shared/TokenLanguageFilter.swift,
TdtDecoderV3.swift:635-703; csrc/tdt_lang.h, csrc/tdt_lang_host.hip): Language, Script, matches, token_classes, topk_rows, decode_logits_lang.

The reference's decoder LSTM and joint network are CoreML bundles that are not part of its source tree, so
``decode_tables`` replays the control loop over tables of the joint's decisions (token, duration bin, probability)
indexed by (decoder steps taken, encoder frame) — token parity against the real models is unpinned."""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass

import numpy as np

from . import _args as A, _lib as L

STANDARD_OVERLAP_FRAMES = 25  # ASRConstants.standardOverlapFrames


@dataclass
class TdtConfig:  # TdtConfig.swift:13-26
    blank_id: int = 8192
    max_symbols_per_step: int = 10
    max_tokens_per_chunk: int = 150
    consecutive_blank_limit: int = 5
    duration_bins: tuple = (0, 1, 2, 3, 4)

    def c(self) -> L.TdtConfig:
        c = L.TdtConfig()
        c.blank_id, c.max_symbols_per_step = self.blank_id, self.max_symbols_per_step
        c.max_tokens_per_chunk, c.consecutive_blank_limit = self.max_tokens_per_chunk, self.consecutive_blank_limit
        c.n_duration_bins = len(self.duration_bins)
        for i, v in enumerate(self.duration_bins):
            c.duration_bins[i] = v
        return c


class TdtFrameNavigation:
    @staticmethod
    def calculate_initial_time_indices(time_jump, context_frame_adjustment: int) -> int:
        return L.lib().fa_tdt_initial_time_index(0 if time_jump is None else 1, 0 if time_jump is None else int(time_jump),
                                                 int(context_frame_adjustment))

    @staticmethod
    def initialize_navigation_state(time_indices: int, encoder_sequence_length: int, actual_audio_frames: int):
        e, s, l, a = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        L.lib().fa_tdt_navigation_state(time_indices, encoder_sequence_length, actual_audio_frames, C.byref(e), C.byref(s),
                                        C.byref(l), C.byref(a))
        return e.value, s.value, l.value, bool(a.value)

    @staticmethod
    def calculate_final_time_jump(current_time_indices: int, effective_sequence_length: int, is_last_chunk: bool):
        has = C.c_int32()
        v = L.lib().fa_tdt_final_time_jump(current_time_indices, effective_sequence_length, int(is_last_chunk), C.byref(has))
        return v if has.value else None


class TdtDurationMapping:
    @staticmethod
    def map_duration_bin(bin_index: int, duration_bins) -> int:
        cfg = TdtConfig(duration_bins=tuple(duration_bins)).c()
        out = C.c_int32()
        if L.lib().fa_tdt_map_duration_bin(C.byref(cfg), int(bin_index), C.byref(out)) != L.SUCCESS:
            raise ValueError(f"Duration bin index out of range: {bin_index}")  # ASRError.processingFailed (:19-21)
        return out.value

    @staticmethod
    def clamp_probability(value: float) -> float:
        return float(L.lib().fa_tdt_clamp_probability(float(value)))


def decode_logits(d_logits, vocab_with_blank: int, enc_len, audio_frames=None, t0=None, is_last=None, global_offset=None, emit_after=None,
                  config: TdtConfig | None = None, max_out: int = 256, ctx: L.Context | None = None):
    """Batched greedy walk on joint LOGITS.  d_logits: a contiguous torch CUDA tensor [B, U, T, W] of float32 or float16 — any other dtype
    is refused, the entry has no code for it — with W >= vocab_with_blank + len(config.duration_bins): a row holds the token logits, the
    duration logits behind them, and W - that many elements of padding the walk never reads.  Its first element may lie at any address a
    tensor of its dtype can have (a view into a larger allocation is fine).  The per-chunk vectors are int sequences, or contiguous int32
    tensors on the logits' device (then nothing is uploaded and the host does not wait for torch's stream).  Same result structure as decode_tables."""
    import torch
    ctx = ctx or L.default_context()
    config = config or TdtConfig()
    cfg = config.c()
    assert isinstance(d_logits, torch.Tensor) and d_logits.is_cuda, "decode_logits: d_logits must be a CUDA tensor"
    assert d_logits.dtype in (torch.float16, torch.float32), f"decode_logits: d_logits must be float16 or float32, not {d_logits.dtype}"
    assert d_logits.dim() == 4, f"decode_logits: d_logits must be [B, U, T, W], not {tuple(d_logits.shape)}"
    B, U, T, W = d_logits.shape
    assert W >= int(vocab_with_blank) + len(config.duration_bins), \
        f"decode_logits: rows of {W} logits cannot hold {int(vocab_with_blank)} token and {len(config.duration_bins)} duration logits"
    assert d_logits.is_contiguous(), "decode_logits: d_logits must be contiguous"
    dev = d_logits.device

    def vec(v):
        return A.to_device(v, np.int32, dev)

    v_enc, v_af, v_t0, v_last, v_go, v_ea = (vec(enc_len), vec(audio_frames), vec(t0), vec(is_last), vec(global_offset),
                                             vec(None if emit_after is None else [-1 if e is None else e for e in emit_after]))
    o_tok, o_time, o_dur = (torch.zeros((B, max_out), dtype=torch.int32, device=dev) for _ in range(3))
    o_conf = torch.zeros((B, max_out), dtype=torch.float32, device=dev)
    o_cnt, o_ft, o_fu, o_st = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    dt = L.DTYPE_F16 if d_logits.dtype == torch.float16 else L.DTYPE_F32
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_tdt_greedy_logits_dev(ctx.handle, C.byref(cfg), p(d_logits), dt, B, U, T, int(vocab_with_blank), W, p(v_enc), p(v_af), p(v_t0),
                                                   p(v_last), p(v_go), p(v_ea), max_out, p(o_tok), p(o_time), p(o_dur), p(o_conf), p(o_cnt), p(o_ft),
                                                   p(o_fu), p(o_st)), "fa_tdt_greedy_logits_dev")
    ctx.synchronize()
    tok, tim, dur, conf = o_tok.cpu().numpy(), o_time.cpu().numpy(), o_dur.cpu().numpy(), o_conf.cpu().numpy()
    cnt, ft, fu, st = o_cnt.cpu().numpy(), o_ft.cpu().numpy(), o_fu.cpu().numpy(), o_st.cpu().numpy()
    out = []
    for b in range(B):
        n = min(int(cnt[b]), max_out)
        out.append(dict(status=int(st[b]), tokens=tok[b, :n].copy(), timestamps=tim[b, :n].copy(), durations=dur[b, :n].copy(),
                        confidences=conf[b, :n].copy(), count=int(cnt[b]), final_time=None if ft[b] == -2 ** 31 else int(ft[b]),
                        final_u=int(fu[b])))
    return out


# ---- language-aware decoding: transcribe(..., language:) (Shared/TokenLanguageFilter.swift, TdtDecoderV3.swift:284-299, 371-387, 635-703)

class Script(enum.IntEnum):  # TokenLanguageFilter.swift:56-60; the values are FA_TDT_SCRIPT_*
    LATIN = 0
    CYRILLIC = 1
    GREEK = 2


class Language(enum.Enum):  # TokenLanguageFilter.swift:4-52
    ENGLISH = "en"
    SPANISH = "es"
    FRENCH = "fr"
    GERMAN = "de"
    ITALIAN = "it"
    PORTUGUESE = "pt"
    ROMANIAN = "ro"
    DUTCH = "nl"
    DANISH = "da"
    SWEDISH = "sv"
    FINNISH = "fi"
    HUNGARIAN = "hu"
    ESTONIAN = "et"
    LATVIAN = "lv"
    LITHUANIAN = "lt"
    MALTESE = "mt"
    POLISH = "pl"
    CZECH = "cs"
    SLOVAK = "sk"
    SLOVENIAN = "sl"
    CROATIAN = "hr"
    BOSNIAN = "bs"
    RUSSIAN = "ru"
    UKRAINIAN = "uk"
    BELARUSIAN = "be"
    BULGARIAN = "bg"
    SERBIAN = "sr"
    GREEK = "el"

    @property
    def script(self) -> Script:
        if self in (Language.RUSSIAN, Language.UKRAINIAN, Language.BELARUSIAN, Language.BULGARIAN, Language.SERBIAN):
            return Script.CYRILLIC
        return Script.GREEK if self is Language.GREEK else Script.LATIN

    @property
    def english_blocklist_applies(self) -> bool:  # TdtDecoderV3.englishBlocklistApplies (:623-625): French only
        return self is Language.FRENCH


CLASS_LATIN_OK, CLASS_CYRILLIC_OK, CLASS_GREEK_OK, CLASS_IN_VOCAB, CLASS_BLOCKLISTED = 1, 2, 4, 8, 16  # FA_TDT_CLASS_*
ROUTE_SCRIPT_SWAP, ROUTE_BLOCKLIST_SWAP = 1, 2                                                         # FA_TDT_ROUTE_*
MAX_TOP_K = 64


def token_classes(vocabulary, blocklist_ids=()) -> np.ndarray:
    """The uint8 class bytes [V1] of fa_tdt_token_classes.  vocabulary: a sequence of V1 texts (None: the id is not in the vocabulary), or a
    dict id -> text with V1 = largest id + 1 (the reference's [Int: String]).  blocklist_ids: the ids the blocklist pass replaces (the product
    ships no list: the reference's is tuned for French, TdtDecoderV3.swift:40-86).  Bits: CLASS_LATIN_OK / CYRILLIC_OK / GREEK_OK = `matches`,
    CLASS_IN_VOCAB, CLASS_BLOCKLISTED.  Raises ValueError for text that is not UTF-8 and for a blocklist id outside the vocabulary."""
    if isinstance(vocabulary, dict):
        n = max(vocabulary) + 1 if vocabulary else 0
        vocabulary = [vocabulary.get(i) for i in range(n)]
    texts = [None if t is None else (t if isinstance(t, bytes) else str(t).encode("utf-8", "surrogatepass")) for t in vocabulary]
    if any(t is not None and b"\0" in t for t in texts):
        raise ValueError("token_classes: a token text holds a NUL")
    V1 = len(texts)
    arr = (C.c_char_p * max(V1, 1))(*texts)
    block = np.ascontiguousarray(list(blocklist_ids), np.int32)
    out = np.zeros(V1, np.uint8)
    st = L.lib().fa_tdt_token_classes(C.cast(arr, C.c_void_p), None, V1, block.ctypes.data if block.size else None, int(block.size),
                                      out.ctypes.data if V1 else None)
    if st != L.SUCCESS:
        raise ValueError("token_classes: a token text is not UTF-8 or a blocklist id lies outside the vocabulary")
    return out


def matches(text: str, script: Script) -> bool:
    """TokenLanguageFilter.matches (TokenLanguageFilter.swift:81-134): every U+2581 scalar is stripped, an empty remainder matches every
    script, the rest is checked scalar by scalar.  A text in which U+2581 is directly followed by a combining mark (U+0300-036F) lies
    outside what the reference's tests pin — Foundation's string search may take the pair for one character and leave the marker in —; this
    library strips the marker there too."""
    return bool(token_classes([text])[0] & (CLASS_LATIN_OK << int(Script(script))))


def topk_rows(d_rows, vocab_with_blank: int, k: int = MAX_TOP_K, ctx: L.Context | None = None):
    """The joint's two top-K outputs as this library defines them (fa_tdt_topk_rows_dev; CoreML leaves the order among equal logits
    open): per row the min(k, vocab_with_blank) tokens in order of descending logit, then ascending id; fp16 is widened, NaN counts as -inf
    and is reported as -inf, -0.0 == +0.0.  d_rows: a contiguous float32 / float16 CUDA tensor [..., W], W >= vocab_with_blank.  Returns
    numpy (ids [..., k] int32, logits [..., k] float32, counts [...] int32); unused slots hold id -1 and logit -inf."""
    import torch
    ctx = ctx or L.default_context()
    assert isinstance(d_rows, torch.Tensor) and d_rows.is_cuda and d_rows.is_contiguous() and d_rows.dim() >= 1, "topk_rows: a contiguous CUDA tensor"
    assert d_rows.dtype in (torch.float16, torch.float32), f"topk_rows: float16 or float32, not {d_rows.dtype}"
    W = d_rows.shape[-1]
    assert 1 <= int(vocab_with_blank) <= W and 1 <= int(k) <= MAX_TOP_K, "topk_rows: 1 <= vocab_with_blank <= row length, 1 <= k <= 64"
    lead = tuple(d_rows.shape[:-1])
    R = int(np.prod(lead, dtype=np.int64))
    ids = torch.zeros((R, k), dtype=torch.int32, device=d_rows.device)
    lg = torch.zeros((R, k), dtype=torch.float32, device=d_rows.device)
    cnt = torch.zeros(R, dtype=torch.int32, device=d_rows.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_tdt_topk_rows_dev(ctx.handle, p(d_rows), L.DTYPE_F16 if d_rows.dtype == torch.float16 else L.DTYPE_F32, R,
                                               int(vocab_with_blank), W, int(k), p(ids), p(lg), p(cnt)), "fa_tdt_topk_rows_dev")
    ctx.synchronize()
    return ids.cpu().numpy().reshape(lead + (k,)), lg.cpu().numpy().reshape(lead + (k,)), cnt.cpu().numpy().reshape(lead)


def decode_logits_lang(d_logits, vocab_with_blank: int, classes, script, enc_len, audio_frames=None, t0=None, is_last=None, global_offset=None,
                       emit_after=None, use_blocklist: bool = False, top_k: int = MAX_TOP_K, config: TdtConfig | None = None, max_out: int = 256,
                       ctx: L.Context | None = None):
    """decode_logits in the reference's language mode (fa_tdt_greedy_logits_lang_dev): at every main-loop and blank-advance decision — never
    in the last-chunk flush — a winner in the wrong script is replaced by the best right-script candidate of the row's top-K list, and with
    use_blocklist a blocklisted label by the best Latin candidate that is neither blank nor blocklisted (Language.english_blocklist_applies
    says when the reference does that).  classes: token_classes(...) [vocab_with_blank] uint8, numpy or a CUDA tensor; script: a Script or a
    Language.  The dicts of decode_logits plus routes (ROUTE_* bits per emitted token) and swap_counts (decisions the script filter / the
    blocklist replaced, emitted or not)."""
    import torch
    ctx = ctx or L.default_context()
    config = config or TdtConfig()
    cfg = config.c()
    script = script.script if isinstance(script, Language) else Script(script)
    assert isinstance(d_logits, torch.Tensor) and d_logits.is_cuda, "decode_logits_lang: d_logits must be a CUDA tensor"
    assert d_logits.dtype in (torch.float16, torch.float32), f"decode_logits_lang: d_logits must be float16 or float32, not {d_logits.dtype}"
    assert d_logits.dim() == 4 and d_logits.is_contiguous(), f"decode_logits_lang: d_logits must be contiguous [B, U, T, W], not {tuple(d_logits.shape)}"
    B, U, T, W = d_logits.shape
    assert W >= int(vocab_with_blank) + len(config.duration_bins), \
        f"decode_logits_lang: rows of {W} logits cannot hold {int(vocab_with_blank)} token and {len(config.duration_bins)} duration logits"
    assert 1 <= int(top_k) <= MAX_TOP_K, f"decode_logits_lang: top_k must be 1 .. {MAX_TOP_K}, not {top_k}"
    dev = d_logits.device
    d_cls = classes if isinstance(classes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(classes, np.uint8))
    d_cls = d_cls.to(dev).contiguous()
    assert d_cls.dtype == torch.uint8 and d_cls.numel() == int(vocab_with_blank), "decode_logits_lang: classes must be vocab_with_blank uint8 bytes"

    def vec(v):
        return A.to_device(v, np.int32, dev)

    v_enc, v_af, v_t0, v_last, v_go, v_ea = (vec(enc_len), vec(audio_frames), vec(t0), vec(is_last), vec(global_offset),
                                             vec(None if emit_after is None else [-1 if e is None else e for e in emit_after]))
    o_tok, o_time, o_dur, o_route = (torch.zeros((B, max_out), dtype=torch.int32, device=dev) for _ in range(4))
    o_conf = torch.zeros((B, max_out), dtype=torch.float32, device=dev)
    o_cnt, o_ft, o_fu, o_st = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
    o_swaps = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    dt = L.DTYPE_F16 if d_logits.dtype == torch.float16 else L.DTYPE_F32
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_tdt_greedy_logits_lang_dev(ctx.handle, C.byref(cfg), p(d_logits), dt, B, U, T, int(vocab_with_blank), W, p(v_enc), p(v_af),
                                                        p(v_t0), p(v_last), p(v_go), p(v_ea), max_out, p(o_tok), p(o_time), p(o_dur), p(o_conf),
                                                        p(o_cnt), p(o_ft), p(o_fu), p(o_st), p(d_cls), int(script), int(bool(use_blocklist)),
                                                        int(top_k), p(o_route), p(o_swaps)), "fa_tdt_greedy_logits_lang_dev")
    ctx.synchronize()
    tok, tim, dur, conf, rt = o_tok.cpu().numpy(), o_time.cpu().numpy(), o_dur.cpu().numpy(), o_conf.cpu().numpy(), o_route.cpu().numpy()
    cnt, ft, fu, st, sw = o_cnt.cpu().numpy(), o_ft.cpu().numpy(), o_fu.cpu().numpy(), o_st.cpu().numpy(), o_swaps.cpu().numpy()
    out = []
    for b in range(B):
        n = min(int(cnt[b]), max_out)
        out.append(dict(status=int(st[b]), tokens=tok[b, :n].copy(), timestamps=tim[b, :n].copy(), durations=dur[b, :n].copy(),
                        confidences=conf[b, :n].copy(), count=int(cnt[b]), final_time=None if ft[b] == -2 ** 31 else int(ft[b]),
                        final_u=int(fu[b]), routes=rt[b, :n].copy(), swap_counts=(int(sw[b, 0]), int(sw[b, 1]))))
    return out


def decode_tables(d_tok, d_bin, d_prob, enc_len, audio_frames=None, t0=None, is_last=None, global_offset=None, emit_after=None,
                  config: TdtConfig | None = None, max_out: int = 256, ctx: L.Context | None = None):
    """Batched greedy walk.  d_tok/d_bin (int32) and d_prob (float32): torch CUDA tensors [B, U, T]; per-chunk int
    sequences for the rest.  Returns a list of dicts (tokens, timestamps, durations, confidences, final_time, final_u, status)."""
    import torch
    ctx = ctx or L.default_context()
    cfg = (config or TdtConfig()).c()
    B, U, T = d_tok.shape
    dev = d_tok.device

    def vec(v):
        return A.to_device(v, np.int32, dev)

    v_enc, v_af, v_t0, v_last, v_go, v_ea = (vec(enc_len), vec(audio_frames), vec(t0), vec(is_last), vec(global_offset),
                                             vec(None if emit_after is None else [-1 if e is None else e for e in emit_after]))
    o_tok, o_time, o_dur = (torch.zeros((B, max_out), dtype=torch.int32, device=dev) for _ in range(3))
    o_conf = torch.zeros((B, max_out), dtype=torch.float32, device=dev)
    o_cnt, o_ft, o_fu, o_st = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    c_tok, c_bin, c_prob = d_tok.contiguous(), d_bin.contiguous(), d_prob.contiguous()   # may launch copies on torch's stream
    with ctx.torch_ordered():
        ctx.check(L.lib().fa_tdt_greedy_tables_dev(ctx.handle, C.byref(cfg), p(c_tok), p(c_bin), p(c_prob),
                                                   B, U, T, p(v_enc), p(v_af), p(v_t0), p(v_last), p(v_go), p(v_ea), max_out, p(o_tok),
                                                   p(o_time), p(o_dur), p(o_conf), p(o_cnt), p(o_ft), p(o_fu), p(o_st)), "fa_tdt_greedy_tables_dev")
    ctx.synchronize()
    tok, tim, dur, conf = o_tok.cpu().numpy(), o_time.cpu().numpy(), o_dur.cpu().numpy(), o_conf.cpu().numpy()
    cnt, ft, fu, st = o_cnt.cpu().numpy(), o_ft.cpu().numpy(), o_fu.cpu().numpy(), o_st.cpu().numpy()
    out = []
    for b in range(B):
        n = min(int(cnt[b]), max_out)
        out.append(dict(status=int(st[b]), tokens=tok[b, :n].copy(), timestamps=tim[b, :n].copy(), durations=dur[b, :n].copy(),
                        confidences=conf[b, :n].copy(), count=int(cnt[b]), final_time=None if ft[b] == -2 ** 31 else int(ft[b]),
                        final_u=int(fu[b])))
    return out
