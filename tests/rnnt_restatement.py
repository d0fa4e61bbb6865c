"""The yardstick of the streaming RNN-T walk and its hotword bias (fa_rnnt_greedy_logits_dev, fa_rnnt_bias_build, fa_rnnt_bias_candidates):
a line-by-line restatement of the reference — NemotronVocabularyBias (Streaming/Nemotron/NemotronVocabularyBias.swift:55-340: pieceForm,
the trie, accumulate, observe, candidates() by its own re-walk of every tail suffix), pickBiased (:482-498) and the greedy loop of
RnntDecoder.decodeWithEOU (Streaming/RnntDecoder.swift:73-127).  On purpose a different algorithm from the device's incremental
matcher.  No GPU, no product code.

What the reference leaves open and this library defines: among candidates of equal score pickBiased takes the lowest token id (the
reference iterates a Dictionary).  What stays with the caller and is therefore not here: the letter-count guard of usableSurfaces."""
import unicodedata

import numpy as np

MARKER = "▁"
DEFAULT_BOOST = 4.5
MAX_BOOST = 6.0
SUCCESS, INVALID_ARGUMENT, OUTPUT_TOO_SMALL, RUNTIME_ERROR = 0, 1, 3, 5
# the Unicode White_Space property
WHITE_SPACE = set([*range(0x09, 0x0E), 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000])


def fold(text):
    return unicodedata.normalize("NFC", text.lower())


def effective_boost(weight, default_boost=DEFAULT_BOOST):   # :196-199
    if weight is None or not weight <= MAX_BOOST:
        return default_boost
    return weight


def is_cjk(ch):   # :219-228
    v = ord(ch)
    return 0x3040 <= v <= 0x30FF or 0x3400 <= v <= 0x4DBF or 0x4E00 <= v <= 0x9FFF or 0xAC00 <= v <= 0xD7AF or 0xF900 <= v <= 0xFAFF


def piece_form(text):   # :233-250
    folded = fold(text)
    anchored = not (folded and is_cjk(folded[0]))
    form, at_boundary = [], True
    for ch in folded:
        if ord(ch) in WHITE_SPACE:
            at_boundary = True
            continue
        if at_boundary:
            if anchored:
                form.append(MARKER)
            at_boundary = False
        form.append(ch)
    return "".join(form)


class TrieNode:
    def __init__(self):
        self.children = {}
        self.entry_indices = []


class Term:
    def __init__(self, text, weight=None, aliases=()):
        self.text, self.weight, self.aliases = text, weight, tuple(aliases)


class VocabularyBias:
    """NemotronVocabularyBias with every surface taken as usable.  pieces: dict id -> piece text (case preserved)."""

    def __init__(self, terms, pieces, default_boost=DEFAULT_BOOST):
        self.entries = []   # (piece form, boost)
        max_len = 0
        for term in terms:
            if not isinstance(term, Term):
                term = Term(term) if isinstance(term, str) else Term(*term)
            boost = effective_boost(term.weight, default_boost)
            if not boost > 0:
                continue
            for surface in (term.text, *term.aliases):
                form = piece_form(surface)
                self.entries.append((form, np.float32(boost)))
                max_len = max(max_len, len(form))
        self.tail_cap = max_len
        self.ids_by_piece, self.piece_by_id = {}, {}
        for i in sorted(pieces):
            piece = pieces[i]
            if piece is None or (piece.startswith("<") and piece.endswith(">")):
                continue
            folded = fold(piece)
            self.ids_by_piece.setdefault(folded, []).append(i)
            self.piece_by_id[i] = folded
        self.root = TrieNode()
        for index, (form, _) in enumerate(self.entries):
            node = self.root
            for ch in form:
                node = node.children.setdefault(ch, TrieNode())
                node.entry_indices.append(index)
        self.fresh = {}
        for entry in self.entries:
            self.accumulate(entry, 0, self.fresh)
        self.tail = []

    @property
    def usable(self):
        return any(form for form, _ in self.entries)   # (a surface of white space alone cannot pass the caller's guard)

    def accumulate(self, entry, offset, best):   # :310-339
        form, boost = entry
        if not offset < len(form):
            return
        piece, letters = "", 0
        for ch in form[offset:]:
            piece += ch
            if ch != MARKER:
                letters += 1
            if piece == MARKER or piece not in self.ids_by_piece:
                continue
            if offset == 0 and form[0] == MARKER and letters < 2:
                continue
            for i in self.ids_by_piece[piece]:
                if boost > best.get(i, -np.inf):
                    best[i] = boost

    def observe(self, token_id):   # :254-261 -> the scalars trimmed from the front
        piece = self.piece_by_id.get(int(token_id))
        if piece is None:
            return 0
        self.tail.extend(piece)
        trimmed = max(0, len(self.tail) - self.tail_cap)
        if trimmed:
            del self.tail[:trimmed]
        return trimmed

    def reset_match_state(self):
        self.tail = []

    def candidates(self):   # :280-306 -> {token id: boost}
        best = dict(self.fresh)
        tail = self.tail
        if tail:
            max_offset = min(len(tail), self.tail_cap)
            for start in range(len(tail) - max_offset, len(tail)):
                node, matched = self.root, True
                for i in range(start, len(tail)):
                    node = node.children.get(tail[i])
                    if node is None:
                        matched = False
                        break
                if not matched:
                    continue
                offset = len(tail) - start
                for index in node.entry_indices:
                    self.accumulate(self.entries[index], offset, best)
        return best

    def live(self):
        """The lengths of the tail's suffixes that are a prefix of some form: the partial matches candidates() continues."""
        out = set()
        for start in range(len(self.tail)):
            node = self.root
            for ch in self.tail[start:]:
                node = node.children.get(ch)
                if node is None:
                    break
            else:
                out.add(len(self.tail) - start)
        return out

    def continuation_only(self):
        """The candidates a fresh start does not offer with at least that boost: what only a live partial match makes possible."""
        return {i: b for i, b in self.candidates().items() if not self.fresh.get(i, -np.inf) >= b}


def argmax_first(row):
    """LogitsArgmax: the first index of the maximum, NaN never wins, nothing above -inf gives 0 (row: float32)."""
    seen = np.where(np.isnan(row), -np.inf, row)
    at = int(np.argmax(seen))            # the first occurrence of the maximum
    return at if seen[at] > -np.inf else 0


def pick_biased(plain, candidates, logits):
    """pickBiased (:482-498) with this library's tie order: the highest score, then the lowest id; a candidate replaces plain only where
    its score is strictly above logit[plain].  logits: float32.  -> the picked id."""
    count = len(logits)
    best_id, best_score = plain, np.float32(logits[plain])
    winner = None
    for i in sorted(candidates):
        if not i < count:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            score = np.float32(np.float32(logits[i]) + np.float32(candidates[i]))
        if score > best_score:        # ascending ids and a strict '>': the lowest id among equal scores
            best_score, best_id, winner = score, i, i
    return best_id if winner is not None else plain


def greedy(logits, V1, frames, skip=0, bias=None, blank_id=None, eou_id=-1, max_symbols=10, max_out=256, trace=None):
    """RnntDecoder.decodeWithEOU (:73-127) on joint logits [U][T][W] (float32 or float16, widened) with selectToken (:465-477) at its
    decision.  bias: a VocabularyBias whose tail is the carried match state (it is advanced), or None.  trace: a list that receives one
    dict per decision: u, t, row (float32), plain, picked, candidates, fresh (the depth-0 candidates), and for an emitted token `dropped`
    (a partial match that was live died on the token's piece without being trimmed away) and `trimmed` (scalars cut at tail_cap).
    Returns what the device entry returns for one stream."""
    U, T = logits.shape[:2]
    blank_id = V1 - 1 if blank_id is None else blank_id
    max_t = max(0, min(int(frames), T))
    start = min(max(0, int(skip)), max_t)
    tokens, tframes, flips = [], [], []
    count = u = 0
    status, eou = SUCCESS, False
    done = False
    for t in range(start, max_t):
        symbols = 0
        while symbols < max_symbols:
            if u >= U:
                status, done = OUTPUT_TOO_SMALL, True
                break
            row = logits[u, t, :V1].astype(np.float32)
            plain = argmax_first(row)
            picked = plain
            cands = {}
            if bias is not None:
                cands = bias.candidates()
                if cands:
                    picked = pick_biased(plain, cands, row)
            event = dict(u=u, t=t, row=row, plain=plain, picked=picked, candidates=dict(cands) if bias is not None else {},
                         fresh=dict(bias.fresh) if bias is not None else {}, emitted=False, dropped=False, trimmed=0)
            if trace is not None:
                trace.append(event)
            if picked == blank_id:
                break
            if picked == eou_id:
                eou, done = True, True
                break
            if count < max_out:
                tokens.append(picked)
                tframes.append(t)
                flips.append(plain if picked != plain else -1)
            else:
                status = OUTPUT_TOO_SMALL
            count += 1
            event["emitted"] = True
            if bias is not None:
                before, grown = bias.live(), len(bias.piece_by_id.get(int(picked), ""))
                event["trimmed"] = bias.observe(picked)
                after = bias.live()
                event["dropped"] = grown > 0 and any(n + grown <= bias.tail_cap and n + grown not in after for n in before)
            u += 1
            symbols += 1
        if done:
            break
    return dict(status=status, tokens=np.asarray(tokens, np.int32), frames=np.asarray(tframes, np.int32), flips=np.asarray(flips, np.int32), count=count,
                final_u=u, eou=eou, tail=np.asarray([ord(c) for c in (bias.tail if bias is not None else [])], np.int32))
