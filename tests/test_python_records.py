"""Every record of the C ABI that Python hands to the library, against a literal table of its layout: the public *_DTYPE names and the
ctypes Structures of _lib.py they are derived from.  The table was written out once from the hand-typed dtypes the package had before the
Structures became the one declaration; it is not computed from the code under test.  No GPU and no library."""
import ctypes as C

import numpy as np
import pytest

import fluidaudio_amd as fa

# (module, public name, Structure in _lib.py): (itemsize, [(field, numpy format, offset)])
RECORDS = {
    ("vad", "VAD_SEGMENT_DTYPE", "VadSegmentRecord"): (40, [("recording", "<i4", 0), ("reserved", "<i4", 4), ("start_sample", "<i8", 8), ("end_sample", "<i8", 16), ("start_time", "<f8", 24), ("end_time", "<f8", 32)]),
    ("vad", "VAD_STREAM_STATE_DTYPE", "VadStreamStateRecord"): (24, [("triggered", "<i4", 0), ("has_temp_end", "<i4", 4), ("temp_end_sample", "<i8", 8), ("processed_samples", "<i8", 16)]),
    ("vad", "VAD_STREAM_EVENT_DTYPE", "VadStreamEventRecord"): (32, [("stream", "<i4", 0), ("chunk", "<i4", 4), ("kind", "<i4", 8), ("reserved", "<i4", 12), ("sample_index", "<i8", 16), ("time", "<f8", 24)]),
    ("tdt_plan", "TDT_WINDOW_DTYPE", "TdtWindowRecord"): (72, [("recording", "<i4", 0), ("use_warmup_prefix", "<i4", 4), ("is_last", "<i4", 8), ("emit_after_frame", "<i4", 12), ("global_frame_offset", "<i4", 16), ("context_frames", "<i4", 20), ("actual_audio_frames", "<i4", 24), ("reserved", "<i4", 28), ("chunk_start", "<i8", 32), ("warmup_samples", "<i8", 40), ("context_samples", "<i8", 48), ("context_start", "<i8", 56), ("length", "<i8", 64)]),
    ("tdt_plan", "TDT_SPAN_DTYPE", "TdtSpanRecord"): (24, [("recording", "<i4", 0), ("reserved", "<i4", 4), ("from_sample", "<i8", 8), ("to_sample", "<i8", 16)]),
    ("paraformer", "PARAFORMER_SPAN_DTYPE", "ParaformerSpan"): (24, [("utterance", "<i4", 0), ("token_index", "<i4", 4), ("start", "<f8", 8), ("end", "<f8", 16)]),
    ("wer", "EDIT_COUNTS_DTYPE", "EditCounts"): (24, [("total", "<i4", 0), ("insertions", "<i4", 4), ("deletions", "<i4", 8), ("substitutions", "<i4", 12), ("hyp_len", "<i4", 16), ("ref_len", "<i4", 20)]),
    ("der", "DER_SEGMENT_DTYPE", "DerSegment"): (24, [("label", "<i4", 0), ("reserved", "<i4", 4), ("start", "<f8", 8), ("end", "<f8", 16)]),
    ("der", "DER_COUNTS_DTYPE", "DerCounts"): (48, [("frames", "<i8", 0), ("miss", "<i8", 8), ("false_alarm", "<i8", 16), ("confusion", "<i8", 24), ("ref", "<i8", 32), ("ref_labels", "<i4", 40), ("hyp_labels", "<i4", 44)]),
    ("kws", "KWS_DETECTION_DTYPE", "KwsDetection"): (20, [("utterance", "<i4", 0), ("keyword", "<i4", 4), ("score", "<f4", 8), ("start_frame", "<i4", 12), ("end_frame", "<i4", 16)]),
    ("kws", "KWS_WINDOW_DTYPE", "KwsWindow"): (16, [("utterance", "<i4", 0), ("keyword", "<i4", 4), ("start_frame", "<i4", 8), ("end_frame", "<i4", 12)]),
    ("timeline", "SEGMENT_DTYPE", "DiarizerSegmentRecord"): (32, [("recording", "<i4", 0), ("speaker", "<i4", 4), ("start_frame", "<i8", 8), ("end_frame", "<i8", 16), ("activity", "<f4", 24), ("finalized", "<i4", 28)]),
    ("sortformer", "SEGMENT_DTYPE", "DiarizerSegmentRecord"): (32, [("recording", "<i4", 0), ("speaker", "<i4", 4), ("start_frame", "<i8", 8), ("end_frame", "<i8", 16), ("activity", "<f4", 24), ("finalized", "<i4", 28)]),
    ("sortformer", "WINDOW_DTYPE", "SortformerWindow"): (32, [("recording", "<i4", 0), ("valid_mel", "<i4", 4), ("valid_out", "<i4", 8), ("first", "<i4", 12), ("mel_start", "<i8", 16), ("g_start", "<i8", 24)]),
    # these five had no Structure before: they name the ones the refactor adds
    ("embedding", "RECORD_DTYPE", "ExportEmbedding"): (32, [("chunk_index", "<i4", 0), ("speaker_index", "<i4", 4), ("start_frame", "<i4", 8), ("end_frame", "<i4", 12), ("start_time", "<f8", 16), ("end_time", "<f8", 24)]),
    ("online", "SPEAKER_ASSIGNMENT_DTYPE", "SpeakerAssignment"): (16, [("id", "<i4", 0), ("slot", "<i4", 4), ("kind", "<i4", 8), ("distance", "<f4", 12)]),
    ("online", "SPEAKER_PAIR_DTYPE", "SpeakerPair"): (20, [("source_id", "<i4", 0), ("destination_id", "<i4", 4), ("source_slot", "<i4", 8), ("destination_slot", "<i4", 12), ("distance", "<f4", 16)]),
    ("online", "ONLINE_RUN_DTYPE", "OnlineRun"): (12, [("stream", "<i4", 0), ("chunk", "<i4", 4), ("local_speaker", "<i4", 8)]),
    ("online", "ONLINE_SEGMENT_DTYPE", "OnlineSegment"): (36, [("stream", "<i4", 0), ("chunk", "<i4", 4), ("local_speaker", "<i4", 8), ("id", "<i4", 12), ("start_frame", "<i4", 16), ("end_frame", "<i4", 20), ("start", "<f4", 24), ("end", "<f4", 28), ("quality", "<f4", 32)]),
}
# the names the package exports at its top level
EXPORTED = ("VAD_SEGMENT_DTYPE", "VAD_STREAM_STATE_DTYPE", "VAD_STREAM_EVENT_DTYPE", "TDT_WINDOW_DTYPE", "TDT_SPAN_DTYPE", "PARAFORMER_SPAN_DTYPE", "EDIT_COUNTS_DTYPE",
            "KWS_DETECTION_DTYPE", "KWS_WINDOW_DTYPE", "SPEAKER_ASSIGNMENT_DTYPE", "SPEAKER_PAIR_DTYPE", "ONLINE_RUN_DTYPE", "ONLINE_SEGMENT_DTYPE")


def layout(dtype):
    return dtype.itemsize, [(n, dtype.fields[n][0].str, dtype.fields[n][1]) for n in dtype.names]


@pytest.mark.parametrize("key", sorted(RECORDS), ids=lambda k: f"{k[0]}.{k[1]}")
def test_public_dtype_matches_the_table(key):
    module, name, _ = key
    dtype = getattr(getattr(fa, module), name)
    assert isinstance(dtype, np.dtype) and layout(dtype) == RECORDS[key]
    if name in EXPORTED:
        assert getattr(fa, name) is dtype


@pytest.mark.parametrize("key", sorted(RECORDS), ids=lambda k: k[2])
def test_structure_matches_the_table(key):
    structure = getattr(fa._lib, key[2])
    assert issubclass(structure, C.Structure) and layout(np.dtype(structure)) == RECORDS[key]
    assert C.sizeof(structure) == RECORDS[key][0] and [f for f, _ in structure._fields_] == [f for f, _, _ in RECORDS[key][1]]


def test_every_exported_dtype_is_in_the_table():
    named = {n for n in dir(fa) if n.endswith("_DTYPE")}
    assert named == set(EXPORTED) and named <= {k[1] for k in RECORDS}


def test_the_segment_record_is_one_object():
    assert fa.timeline.SEGMENT_DTYPE is fa.sortformer.SEGMENT_DTYPE
