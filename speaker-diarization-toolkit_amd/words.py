"""Speaker-attributed transcripts: the words of a speech-to-text transcript onto the per-frame speakers of a diarization
(diarize.DiarizationResult.speakers), and the word-level diarization error rate (WDER) of the result against the labels a transcript
already carries (backend.attribute_transcript / attribute_transcripts / diarize_transcript / score_words, functions of backend.py).  The rule below is THIS build's
statement; no other toolkit's code is on hand, so PARITY IS UNPINNED and the tests pin this rule.

  grid        that of score.py: frame g of a recording has centre sample 270 g + 495, g < G = global_frames(n_samples).  The hypothesis on
              it is a result's speakers [G, 2] (int32, padded with -1): speaker k is active in frame g iff k stands in speakers[g].  An
              entry < 0 or >= K_r (the result's n_speakers) names nobody; a speaker named twice in a frame counts once
  words       per recording an ordered list of (start_s, end_s); seconds to samples by floor(t * 16000 + 0.5), as score.prepare_reference
              (prepare_words).  Times must be finite, >= 0 and below 2^31 samples: anything else is a ValueError that names the word
  frames      of a word (s0, s1): g0 = clamp(ceil((s0 - 495) / 270), 0, G), g1 = clamp(ceil((s1 - 495) / 270), 0, G) - the frames whose
              centre lies in [s0, s1).  If g1 <= g0 (a zero-length word, one shorter than a hop between two centres, one before frame 0 or
              past the end): the one frame whose centre is nearest the midpoint m = (s0 + s1) >> 1: g0 = clamp(floor((m - 360) / 270), 0,
              G - 1), g1 = g0 + 1.  G == 0: the word gets speaker -1, every count 0 and distance -1.  span = g1 - g0
  votes       v[k] = the frames of the word in which k is active, u[k] = those in which k is the only active speaker
  winner      the k with v[k] > 0 that is first in the order (v descending, then u descending, then k ascending); second = the next in that
              order with v > 0, else -1; distance = 0
  fallback    every v is 0 (the word lies in non-speech): with gap = floor(max_gap_s * 16000 + 0.5) // 270 frames (max_gap_s 0.5 by
              default), the least d in 1 .. gap for which frame g0 - d or frame g1 - 1 + d names somebody - both inside [0, G) of the
              word's OWN recording, never a neighbour's in a pack; at equal d the earlier side wins, inside the frame the first entry that
              names somebody.  The word gets that speaker with votes 0 and distance = d; no such frame: speaker -1, distance -1
  row         per word [8] int32: (speaker, votes, solo, span, second, second_votes, distance, g0), g0 local to the recording
  limits      at most MAX_WORD_SPEAKERS = 1024 hypothesis speakers per recording: more is a ValueError here and refused by the library.
              Every count is below 2^31

  WDER        a word is scored when its reference label is a known speaker (not None, not "UU"); reference names are numbered by first
              appearance.  co[i, j] = the scored words with reference i and hypothesis j (a hypothesis of -1 falls in no column);
              correct = the exact maximum-weight assignment on co (score.py's "mapping", on the word table instead of the frame table);
              wder = 1 - correct / scored, 0.0 when scored == 0.  unassigned = the scored words with hypothesis -1 (they count as errors).
              Pooled over recordings (pool): the ratio of the sums.  At most score.MAX_SCORE_SPEAKERS = 64 speakers a side

The device path (csrc/words.hip) is one launch for a pack of recordings on the prefix-sum tables of diarize_ops.GroupTables:
sdk_words_attribute, one wave per word, the votes in LDS; then sdk_words_cooccur (rows and reference labels -> co and the tallies, summed
per workgroup in LDS, then integer atomics) and score.py's sdk_score_map unchanged.  Integers only: bit-identical run to run.  attribute_host
and wder_host restate them in numpy.

The transcript side reads and writes three layouts: Speechmatics (`results` items of type word / punctuation), AssemblyAI (`utterances[*].words`,
milliseconds) and OpenAI verbose_json (`words [{word, start, end}]`), the last one written back in the Speechmatics layout, which
segments.py and assign.py read.
"""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass
from typing import TYPE_CHECKING, Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .score import FRAME_FIRST, MAX_SCORE_SPEAKERS, _check_counts, _first_frame, assignment_host
from .segmentation import FRAME_HOP, SAMPLE_RATE
from .segments import UNKNOWN_SPEAKER, detect_transcript_format

if TYPE_CHECKING:
    from .backend import Backend

MAX_WORD_SPEAKERS = 1024
DEFAULT_MAX_GAP_S = 0.5
ROW_FIELDS = ("speaker", "votes", "solo", "span", "second", "second_votes", "distance", "g0")
_BIG = 1 << 40


@dataclass
class WordLabels:
    """The attribution of one recording's words: rows [W, 8] int32, a column per ROW_FIELDS name."""
    rows: np.ndarray

    def __getattr__(self, name):
        if name in ROW_FIELDS:
            return self.rows[:, ROW_FIELDS.index(name)]
        raise AttributeError(name)

    def __len__(self) -> int:
        return int(self.rows.shape[0])


@dataclass
class WderResult:
    scored: int                               # words with a known reference speaker
    unassigned: int                           # scored words without a hypothesis speaker (errors)
    words: int                                # all words
    correct: int
    wder: float
    mapping: Dict[object, int]                # reference name -> hypothesis speaker, -1: unmapped ({} for a pooled result)
    co: Optional[np.ndarray]                  # [S, K] int32 (None for a pooled result)


def wder_value(scored: int, correct: int) -> float:
    return 0.0 if int(scored) == 0 else 1.0 - int(correct) / int(scored)


def pool(results: Sequence[WderResult]) -> WderResult:
    """The summed tallies of many recordings and the ratio of the sums; mapping {} and co None (not comparable across recordings)."""
    s = [sum(int(getattr(r, f)) for r in results) for f in ("scored", "unassigned", "words", "correct")]
    return WderResult(*s, wder_value(s[0], s[3]), {}, None)


# ------------------------------------------------------------------------------------------------ the rule on the host
def gap_frames(max_gap_s: float) -> int:
    if not (max_gap_s == max_gap_s and 0.0 <= max_gap_s and max_gap_s * SAMPLE_RATE + 0.5 < float(1 << 30)):
        raise ValueError(f"words: max_gap_s={max_gap_s} (seconds, >= 0)")
    return int(math.floor(float(max_gap_s) * SAMPLE_RATE + 0.5)) // FRAME_HOP


def prepare_words(words) -> np.ndarray:
    """[(start_s, end_s, ...)] -> [W, 2] int32 samples: "words" in the module docstring."""
    out = np.zeros((len(words), 2), np.int32)
    for i, word in enumerate(words):
        for c in (0, 1):
            t = float(word[c])
            if not (t == t and 0.0 <= t and t * SAMPLE_RATE + 0.5 < float(1 << 31)):
                raise ValueError(f"words: word {i} ({word[0]!r} .. {word[1]!r} s): times must be finite, >= 0 and below 2^31 samples")
            out[i, c] = int(math.floor(t * SAMPLE_RATE + 0.5))
    return out


def _check_speakers(who: str, K: int):
    if K > MAX_WORD_SPEAKERS:
        raise ValueError(f"{who}: {K} hypothesis speakers; at most {MAX_WORD_SPEAKERS} per recording")


def attribute_host(speakers, K: int, words: np.ndarray, gap: int) -> np.ndarray:
    """sdk_words_attribute for one recording in numpy: speakers [G, 2], its K speakers, words [W, 2] in samples (prepare_words), gap in
    frames (gap_frames) -> rows [W, 8] int32.  Vectorised over words: the votes are differences of per-speaker prefix sums over the frames,
    the fallback reads the nearest voiced frame on either side from two running extrema."""
    sp = np.asarray(speakers, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(words, dtype=np.int64).reshape(-1, 2)
    G, W, K = sp.shape[0], w.shape[0], max(int(K), 0)
    _check_speakers("attribute_host", K)
    rows = np.zeros((W, 8), np.int32)
    rows[:, [0, 4, 6]] = -1
    if G == 0 or W == 0:
        return rows
    h0, h1 = sp[:, 0], sp[:, 1]
    ok0, in1 = (h0 >= 0) & (h0 < K), (h1 >= 0) & (h1 < K)
    ok1 = in1 & (h1 != h0)
    g0, g1 = np.minimum(_first_frame(w[:, 0]), G), np.minimum(_first_frame(w[:, 1]), G)
    point = g1 <= g0
    mid = np.clip((((w[:, 0] + w[:, 1]) >> 1) - (FRAME_FIRST - FRAME_HOP // 2)) // FRAME_HOP, 0, G - 1)
    g0, g1 = np.where(point, mid, g0), np.where(point, mid + 1, g1)
    rows[:, 3], rows[:, 7] = g1 - g0, g0
    has = np.zeros(W, bool)
    ids = np.unique(np.concatenate([h0[ok0], h1[ok1]]))                                  # the speakers that appear, ascending
    if ids.size:
        act, solo = np.zeros((G + 1, ids.size), np.int64), np.zeros((G + 1, ids.size), np.int64)
        act[np.nonzero(ok0)[0] + 1, np.searchsorted(ids, h0[ok0])] = 1
        act[np.nonzero(ok1)[0] + 1, np.searchsorted(ids, h1[ok1])] = 1
        one = ok0 != ok1
        solo[np.nonzero(one)[0] + 1, np.searchsorted(ids, np.where(ok0, h0, h1)[one])] = 1
        cv, cu = np.cumsum(act, 0), np.cumsum(solo, 0)
        v, u = cv[g1] - cv[g0], cu[g1] - cu[g0]                                          # [W, P]
        key = np.where(v > 0, (v << 31) | u, -1)                                         # argmax: the first maximum, the least k
        ar = np.arange(W)
        b = key.argmax(1)
        has = key[ar, b] >= 0
        rows[has, 0], rows[has, 1], rows[has, 2], rows[has, 6] = ids[b[has]], v[ar, b][has], u[ar, b][has], 0
        key[ar, b] = -1
        b2 = key.argmax(1)
        has2 = has & (key[ar, b2] >= 0)
        rows[has2, 4], rows[has2, 5] = ids[b2[has2]], v[ar, b2][has2]
    voiced, idx = ok0 | in1, np.arange(G)
    first = np.where(ok0, h0, h1)
    prev = np.maximum.accumulate(np.where(voiced, idx, -1))                              # the last voiced frame <= g
    nxt = np.minimum.accumulate(np.where(voiced, idx, _BIG)[::-1])[::-1]                 # the first voiced frame >= g
    e = np.where(g0 >= 1, prev[np.maximum(g0 - 1, 0)], -1)
    la = np.where(g1 <= G - 1, nxt[np.minimum(g1, G - 1)], _BIG)
    de, dl = np.where(e >= 0, g0 - e, _BIG), np.where(la < _BIG, la - (g1 - 1), _BIG)
    d = np.minimum(de, dl)
    fb = ~has & (d <= int(gap))
    at = np.where(de <= dl, e, la)
    rows[fb, 0], rows[fb, 6] = first[np.clip(at, 0, G - 1)][fb], d[fb]
    return rows


def _reference_ids(labels) -> Tuple[np.ndarray, list]:
    """Per word a reference label (None and "UU": not scored) -> (ids [W] int32, -1: not scored; names by first appearance)."""
    names: Dict[object, int] = {}
    ids = np.full(len(labels), -1, np.int32)
    for i, lab in enumerate(labels):
        if lab is None or lab == UNKNOWN_SPEAKER:
            continue
        ids[i] = names.setdefault(lab, len(names))
    return ids, list(names)


def _wder_result(names, co, tally, mapping, correct) -> WderResult:
    scored, unassigned, words = (int(x) for x in tally)
    return WderResult(scored, unassigned, words, int(correct), wder_value(scored, correct), {name: int(mapping[i]) for i, name in enumerate(names)},
                      np.asarray(co, dtype=np.int32))


def wder_host(hyp, reference, K: Optional[int] = None) -> WderResult:
    """One recording on the host: hyp [W] the words' speakers (-1: none; rows[:, 0]), reference [W] their reference labels, K the
    hypothesis speakers (default: the largest named, plus one) -> WderResult."""
    hyp = np.asarray(hyp, dtype=np.int64).reshape(-1)
    if len(reference) != hyp.size:
        raise ValueError(f"wder_host: {len(reference)} reference labels for {hyp.size} words")
    ids, names = _reference_ids(reference)
    K = (int(hyp.max()) + 1 if hyp.size else 0) if K is None else int(K)
    S, K = len(names), max(K, 0)
    _check_counts("wder_host", S, K)
    scored = ids >= 0
    on = scored & (hyp >= 0) & (hyp < K)
    co = np.zeros((S, K), np.int32)
    np.add.at(co, (ids[on], hyp[on]), 1)
    mapping, correct = assignment_host(co) if S and K else (np.full(S, -1, np.int32), 0)
    return _wder_result(names, co, (scored.sum(), (scored & ~on).sum(), hyp.size), mapping, correct)


# ------------------------------------------------------------------------------------------------ the device path
class WordPack:
    """A pack's words attributed on the device (attribute_pack): what wder_pack reads without another upload."""
    R: int
    word_off: np.ndarray         # [R + 1] int64
    cent_off: np.ndarray         # [R + 1] int64
    word_off_d = None            # [R + 1] int32
    cent_off_d = None
    rows = None                  # [W, 8] int32 on the device


def _ops():
    import torch
    from . import ops_score
    from ._lib import check
    from .ops_util import _stream
    return torch, ops_score, check, _stream


def attribute_pack(eng, results, words_per_recording, max_gap_s: float = DEFAULT_MAX_GAP_S) -> WordPack:
    """DiarizationResults (their speakers and n_speakers are read) and one word list [(start_s, end_s, ...)] per result -> WordPack: the
    words and their prefix sums in one upload, the hypothesis uploaded as score.score_results uploads it, one launch."""
    from .diarize_ops import GroupTables
    torch, ops_score, _, _ = _ops()
    results, word_lists = list(results), list(words_per_recording)
    if len(word_lists) != len(results) or not results:
        raise ValueError(f"words: {len(word_lists)} word lists for {len(results)} recordings (one each, at least one)")
    spk = [np.ascontiguousarray(res.speakers, dtype=np.int32).reshape(-1, 2) for res in results]
    for r, res in enumerate(results):
        _check_speakers(f"words: recording {r}", int(res.n_speakers))
    gap = gap_frames(max_gap_s)
    samples = [prepare_words(w) for w in word_lists]
    pack = WordPack()
    pack.R = R = len(results)
    pack.word_off = np.concatenate([[0], np.cumsum([len(s) for s in samples])]).astype(np.int64)
    if pack.word_off[-1] >= (1 << 28):
        raise ValueError(f"words: {int(pack.word_off[-1])} words in one pack (fewer than 2^28)")
    G_r = [len(sp) for sp in spk]
    n_samples = [FRAME_HOP * g + 226 if g else 0 for g in G_r]                      # a length with global_frames(n) == g: only the grid is read
    tab = GroupTables(eng, np.zeros(R + 1, np.int64), np.concatenate([[0], np.cumsum(G_r)]), n_samples)
    tab.set_clusters(np.concatenate([[0], np.cumsum([max(int(res.n_speakers), 0) for res in results])]))
    pack.cent_off, pack.cent_off_d = tab.cent_off, tab.cent_off_d
    up = torch.from_numpy(np.concatenate([pack.word_off.astype(np.int32)] + [s.reshape(-1) for s in samples])).to(eng.device)     # one upload
    pack.word_off_d, words_d = up[:R + 1], up[R + 1:].reshape(-1, 2)
    speakers_d = torch.from_numpy(np.concatenate(spk)).to(eng.device)
    max_hyp = int(np.diff(tab.cent_off).max())
    pack.rows = ops_score.words_attribute(eng, words_d, pack.word_off_d, speakers_d, tab.frame_off_d, tab.cent_off_d, max_hyp, gap)
    return pack


def _split_rows(rows: np.ndarray, word_off) -> List[WordLabels]:
    return [WordLabels(rows[int(a):int(b)]) for a, b in zip(word_off[:-1], word_off[1:])]


def attribute(eng, results, words_per_recording, max_gap_s: float = DEFAULT_MAX_GAP_S) -> List[WordLabels]:
    """A pack of recordings in one upload and one launch (attribute_pack), then one download -> one WordLabels per recording."""
    pack = attribute_pack(eng, results, words_per_recording, max_gap_s)
    return _split_rows(pack.rows.cpu().numpy(), pack.word_off)


def wder_pack(eng, pack: WordPack, references) -> List[WderResult]:
    """The words of a WordPack against their reference labels (one list per recording, a label per word; None and "UU": not scored) -> one
    WderResult per recording: sdk_words_cooccur, sdk_score_map, one download."""
    torch, ops_score, check, _stream = _ops()
    references = list(references)
    if len(references) != pack.R:
        raise ValueError(f"wder: {len(references)} reference lists for {pack.R} recordings")
    prepared = []
    for r, labels in enumerate(references):
        if len(labels) != int(pack.word_off[r + 1] - pack.word_off[r]):
            raise ValueError(f"wder: recording {r}: {len(labels)} reference labels for {int(pack.word_off[r + 1] - pack.word_off[r])} words")
        prepared.append(_reference_ids(labels))
    S_r, K_r = np.asarray([len(n) for _, n in prepared], np.int64), np.diff(pack.cent_off)
    for r in range(pack.R):
        _check_counts(f"wder: recording {r}", int(S_r[r]), int(K_r[r]))
    R = pack.R
    ref_off = np.concatenate([[0], np.cumsum(S_r)]).astype(np.int64)
    co_off = np.concatenate([[0], np.cumsum(S_r * K_r)]).astype(np.int64)
    n_ref, total, W = int(ref_off[-1]), int(co_off[-1]), int(pack.word_off[-1])
    up = torch.from_numpy(np.concatenate([ref_off.astype(np.int32)] + [ids for ids, _ in prepared])).to(eng.device)
    ref_off_d, ref_d = up[:R + 1], up[R + 1:]
    co_off_d = torch.from_numpy(co_off).to(eng.device)
    max_ref, max_hyp = int(S_r.max()), int(K_r.max())
    co, tally = ops_score.words_cooccur(eng, pack.rows, ref_d, pack.word_off_d, ref_off_d, pack.cent_off_d, co_off_d, max_ref, max_hyp, total)
    mapping = torch.empty((max(n_ref, 1),), dtype=torch.int32, device=eng.device)
    correct = torch.empty((R,), dtype=torch.int64, device=eng.device)
    check(eng.lib.sdk_score_map(eng.ctx, co.data_ptr(), ref_off_d.data_ptr(), pack.cent_off_d.data_ptr(), co_off_d.data_ptr(), R, max_ref,
                                max_hyp, mapping.data_ptr(), correct.data_ptr(), _stream()), "sdk_score_map")
    flat = torch.cat([tally.reshape(-1), correct, mapping[:n_ref].to(torch.int64), co[:total].to(torch.int64)]).cpu().numpy()
    tal, cor, mp, cof = flat[:3 * R].reshape(R, 3), flat[3 * R:4 * R], flat[4 * R:4 * R + n_ref], flat[4 * R + n_ref:]
    out = []
    for r, (_, names) in enumerate(prepared):
        S, K, a = len(names), int(K_r[r]), int(co_off[r])
        out.append(_wder_result(names, cof[a:a + S * K].reshape(S, K), tal[r], mp[int(ref_off[r]):int(ref_off[r + 1])], cor[r]))
    return out


def wder(eng, results, words_per_recording, references, max_gap_s: float = DEFAULT_MAX_GAP_S) -> List[WderResult]:
    """attribute_pack, then wder_pack: the attribution of every recording's words scored against their reference labels, on the device."""
    return wder_pack(eng, attribute_pack(eng, results, words_per_recording, max_gap_s), references)


# ------------------------------------------------------------------------------------------------ the transcript side
Word = Tuple[float, float, str, Optional[str]]


def transcript_layout(data: Dict[str, Any]) -> str:
    """'speechmatics' | 'assemblyai' | 'openai'; anything else is a ValueError."""
    fmt = detect_transcript_format(data) if isinstance(data, dict) else "unknown"
    if fmt in ("assemblyai", "speechmatics"):
        return fmt
    words = data.get("words") if isinstance(data, dict) else None
    if isinstance(words, list) and all(isinstance(w, dict) and "word" in w and "start" in w and "end" in w for w in words) and (words or "text" in data):
        return "openai"
    raise ValueError("words: unknown transcript layout (Speechmatics `results`, AssemblyAI `utterances` or OpenAI verbose_json `words` expected)")


def _aai_words(data) -> List[Tuple[Dict[str, Any], Optional[str]]]:
    """AssemblyAI: every word dict with its speaker (its own, else its utterance's), in order; an utterance without words takes the
    top-level words that start inside it."""
    out = []
    top = data.get("words") or []
    for u in data.get("utterances", []):
        ws = u.get("words")
        if not ws:
            ws = [w for w in top if u.get("start", 0) <= w.get("start", 0) < u.get("end", 0)]
        out += [(w, w.get("speaker") or u.get("speaker")) for w in ws]
    return out


def transcript_words(data: Dict[str, Any]) -> List[Word]:
    """A transcript -> [(start_s, end_s, text, reference_speaker_or_None)] in document order."""
    layout = transcript_layout(data)
    if layout == "speechmatics":
        out = []
        for item in data.get("results", []):
            if item.get("type") != "word":
                continue
            alts = item.get("alternatives", [])
            spk = item.get("speaker") or (alts[0].get("speaker") if alts else None)
            out.append((item.get("start_time", 0), item.get("end_time", 0), alts[0].get("content", "") if alts else "", spk))
        return out
    if layout == "assemblyai":
        return [(w.get("start", 0) / 1000.0, w.get("end", 0) / 1000.0, w.get("text", ""), spk) for w, spk in _aai_words(data)]
    return [(w["start"], w["end"], str(w["word"]).strip(), None) for w in data["words"]]


def _labels(speakers, names, n_words: int) -> List[str]:
    spk = np.asarray(speakers.rows if isinstance(speakers, WordLabels) else speakers)
    if spk.ndim == 2:
        spk = spk[:, 0]
    if spk.shape != (n_words,):
        raise ValueError(f"words: {spk.shape[0] if spk.ndim else 0} speakers for the transcript's {n_words} words")
    out = []
    for k in spk.tolist():
        if k < 0:
            out.append(UNKNOWN_SPEAKER)
        elif names is None:
            out.append(f"S{int(k) + 1}")
        else:
            if k >= len(names):
                raise ValueError(f"words: speaker {k} has no name ({len(names)} names)")
            out.append(names[int(k)])
    return out


def relabel_transcript(data: Dict[str, Any], speakers, names=None) -> Dict[str, Any]:
    """A deep copy of the transcript in which every word carries its new speaker: speakers [W] (or rows [W, 8], or a WordLabels) in the
    order of transcript_words; speaker k is "S<k+1>", or names[k]; -1 is "UU".  Speechmatics: set on the item and in alternatives[0],
    punctuation takes the preceding word's.  AssemblyAI: the utterances are regrouped at speaker changes.  OpenAI: returned as a
    Speechmatics-layout document."""
    layout = transcript_layout(data)
    if layout == "speechmatics":
        out = copy.deepcopy(data)
        items = [it for it in out.get("results", []) if it.get("type") == "word"]
        labs = _labels(speakers, names, len(items))
        i, last = 0, None
        for item in out.get("results", []):
            if item.get("type") == "word":
                last = labs[i]
                i += 1
            elif item.get("type") != "punctuation" or last is None:
                continue
            item["speaker"] = last
            if item.get("alternatives"):
                item["alternatives"][0]["speaker"] = last
        return out
    if layout == "assemblyai":
        pairs = _aai_words(data)
        labs = _labels(speakers, names, len(pairs))
        out = copy.deepcopy({k: v for k, v in data.items() if k not in ("utterances", "words")})
        utts: List[Dict[str, Any]] = []
        for (w, _), lab in zip(pairs, labs):
            w = dict(copy.deepcopy(w), speaker=lab)
            if utts and utts[-1]["speaker"] == lab:
                utts[-1]["words"].append(w)
            else:
                utts.append({"speaker": lab, "words": [w]})
        for u in utts:
            u["start"], u["end"] = u["words"][0].get("start", 0), u["words"][-1].get("end", 0)
            u["text"] = " ".join(w.get("text", "") for w in u["words"] if w.get("text"))
        out["utterances"] = utts
        if "words" in data:
            out["words"] = [w for u in utts for w in u["words"]]
        return out
    labs = _labels(speakers, names, len(data["words"]))
    results = [{"type": "word", "start_time": w["start"], "end_time": w["end"], "speaker": lab,
                "alternatives": [{"content": str(w["word"]).strip(), "speaker": lab}]} for w, lab in zip(data["words"], labs)]
    meta = {k: data[k] for k in ("language", "duration") if k in data}
    return {"format": "2.9", "metadata": dict(meta, source="openai verbose_json"), "results": results}


def attributed_sentences(data: Dict[str, Any], rows) -> List[Dict[str, Any]]:
    """A transcript and its words' rows [W, 8] (or a WordLabels) -> [{speaker, start, end, text, words, min_votes_share}]: a sentence ends
    at Speechmatics `is_eos` punctuation and at every change of the attributed speaker (-1: nobody).  min_votes_share: the least
    votes / span of its words - 0.0 for a word attributed by the fallback."""
    rows = np.asarray(rows.rows if isinstance(rows, WordLabels) else rows).reshape(-1, 8)
    words = transcript_words(data)
    if len(words) != rows.shape[0]:
        raise ValueError(f"words: {rows.shape[0]} rows for the transcript's {len(words)} words")
    tokens: List[Tuple[str, Any]] = []
    if transcript_layout(data) == "speechmatics":
        i = 0
        for item in data.get("results", []):
            if item.get("type") == "word":
                tokens.append(("word", i))
                i += 1
            elif item.get("type") == "punctuation":
                alts = item.get("alternatives", [])
                tokens.append(("eos" if item.get("is_eos") else "mark", alts[0].get("content", "") if alts else ""))
    else:
        tokens = [("word", i) for i in range(len(words))]
    out: List[Dict[str, Any]] = []
    cur = None
    for kind, val in tokens:
        if kind == "word":
            s, e, text, _ = words[val]
            spk, votes, span = int(rows[val, 0]), int(rows[val, 1]), int(rows[val, 3])
            share = votes / span if span > 0 else 0.0
            if cur is not None and cur["speaker"] != spk:
                out.append(cur)
                cur = None
            if cur is None:
                cur = {"speaker": spk, "start": s, "end": e, "text": text, "words": 1, "min_votes_share": share}
            else:
                cur["end"], cur["words"], cur["min_votes_share"] = e, cur["words"] + 1, min(cur["min_votes_share"], share)
                cur["text"] = (cur["text"] + " " + text).strip()
        elif cur is not None:
            cur["text"] += val
            if kind == "eos":
                out.append(cur)
                cur = None
    if cur is not None:
        out.append(cur)
    return out


# ---- the functions of a Backend (backend.py) on words: not methods of it, whose public surface is pinned name for name
#      (tests/test_rules_cpu.py); backend.py imports them, so callers reach them as backend.attribute_transcripts and so on.
def attribute_transcripts(be: Backend, results, transcripts, max_gap_s: float = 0.5, names=None):
    """Who said which word: the results of diarize / diarize_many / a finished stream and one word-timed transcript per result (dicts in
    the Speechmatics, AssemblyAI or OpenAI verbose_json layout; the speakers they carry are not read) -> a list of (relabelled, rows):
    the transcript relabelled in its own layout (OpenAI: in the Speechmatics layout) with speaker k as "S<k+1>", or names[k], or "UU"
    for a word nobody is near, and rows [W, 8] int32 per word (speaker, votes, solo, span, second, second_votes, distance, g0).  A word
    goes to the speaker active in most of its frames; a word in non-speech to the nearest voiced frame within max_gap_s.  All words of
    all recordings are attributed in one launch on the device (words.py states the rule; parity with other toolkits is unpinned).
    relabelled feeds segments.sentence_segments, extract_segments_as_tuples and assign.py; words.attributed_sentences(transcript,
    rows) gives the sentences with their text."""
    from . import words as wd
    results, transcripts = list(results), list(transcripts)
    if len(transcripts) != len(results):
        raise ValueError(f"attribute_transcripts: {len(transcripts)} transcripts for {len(results)} recordings")
    if not results:
        return []
    labels = wd.attribute(be.engine(), results, [wd.transcript_words(t) for t in transcripts], max_gap_s)
    return [(wd.relabel_transcript(t, lab.rows, names), lab.rows) for t, lab in zip(transcripts, labels)]


def attribute_transcript(be: Backend, result, transcript, max_gap_s: float = 0.5, names=None):
    """attribute_transcripts for one recording -> (relabelled, rows)."""
    return attribute_transcripts(be, [result], [transcript], max_gap_s, names)[0]


def diarize_transcript(be: Backend, samples_or_path, transcript, max_gap_s: float = 0.5, names=None, **diarize_keywords):
    """diarize, then attribute_transcript: a recording and its word-timed transcript (say OpenAI/Whisper verbose_json, which has no
    speakers) -> (relabelled, rows, result): the transcript with a speaker on every word, the words' rows and the
    diarize.DiarizationResult they were read from.  diarize_keywords: those of diarize."""
    result = be.diarize(samples_or_path, **diarize_keywords)
    relabelled, rows = attribute_transcript(be, result, transcript, max_gap_s, names)
    return relabelled, rows, result


def score_words(be: Backend, results, transcripts, max_gap_s: float = 0.5):
    """How good the attribution is: the word-level diarization error rate (WDER) of attribute_transcripts against the speakers the
    transcripts already carry -> (a list of words.WderResult (scored, unassigned, words, correct, wder, mapping, co), the pooled
    WderResult).  A word is scored when the transcript gives it a speaker other than "UU"; the hypothesis speakers are mapped onto the
    reference's by the exact maximum-weight assignment, and a scored word without a speaker is an error.  Attributed and scored on
    the device in one pack (words.py states the rule; parity with other toolkits is unpinned)."""
    from . import words as wd
    results, transcripts = list(results), list(transcripts)
    if len(transcripts) != len(results):
        raise ValueError(f"score_words: {len(transcripts)} transcripts for {len(results)} recordings")
    if not results:
        return [], wd.pool([])
    words = [wd.transcript_words(t) for t in transcripts]
    per = wd.wder(be.engine(), results, words, [[w[3] for w in ws] for ws in words], max_gap_s)
    return per, wd.pool(per)
