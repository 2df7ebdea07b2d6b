"""Arrow record input for the multi-label task.

Reference: MultiArrowGenerator (rust/src/tasks/multi_label/multi_arrow.rs:11-41)
turns each Arrow row into a SimpleTransport {text: sentence, label:
Label::Multi(labels)} one `slice(0,1)` at a time, and ArrowTransfer
(rust/src/provider/arrow_transfer.rs:48-118) streams the record batches.

Here the same schema (`sentence: utf8`, `labels: list<int64>`) is read with
pyarrow and a whole record batch becomes the Batcher's text arena without a
per-row copy: the utf8 column's value buffer IS the arena and its int32 offsets
become the uint64 record offsets; the list column's offsets/values become the
Label::Multi index arrays.  `MultiArrowGenerator.get_data` keeps the
reference's per-row form for callers that want SimpleTransport objects.
"""
from dataclasses import dataclass
from typing import Iterator

import numpy as np

from .batcher import Label, SimpleData, SimpleTransport


def _pa():
    import pyarrow as pa  # host-side dependency of the Arrow provider only
    return pa


def read_stream(source) -> Iterator["pyarrow.RecordBatch"]:  # noqa: F821
    """Record batches of an Arrow IPC stream (path, bytes or file-like)."""
    pa = _pa()
    if isinstance(source, (bytes, bytearray, memoryview)):
        source = pa.BufferReader(source)
    with pa.ipc.open_stream(source) as r:
        for b in r:
            yield b


class MultiArrowGenerator:
    """ArrowGenerator for multi-label rows (multi_arrow.rs:11-41)."""

    def __init__(self, schema):
        self.t = schema.get_field_index("sentence")
        self.l = schema.get_field_index("labels")
        if self.t < 0 or self.l < 0:
            raise KeyError("schema needs `sentence` and `labels` columns")  # reference: unwrap() panics

    def get_data(self, batch, row: int = 0) -> SimpleTransport:
        text = batch.column(self.t)[row].as_py()
        labels = [int(x) for x in batch.column(self.l)[row].as_py()]
        return SimpleTransport(SimpleData(text, None), Label(multi=labels))


class SingleClassArrowGenerator:
    """ArrowGenerator for single-class rows (single_class/single_arrow.rs:11-39):
    `text` utf8 + `label` int64 -> SimpleTransport with Label::Single(label as u32)."""

    def __init__(self, schema):
        self.t = schema.get_field_index("text")
        self.l = schema.get_field_index("label")
        if self.t < 0 or self.l < 0:
            raise KeyError("schema needs `text` and `label` columns")  # reference: unwrap() panics

    def get_data(self, batch, row: int = 0) -> SimpleTransport:
        text = batch.column(self.t)[row].as_py()
        label = int(batch.column(self.l)[row].as_py()) & 0xFFFFFFFF  # `as u32`
        return SimpleTransport(SimpleData(text, None), Label(single=label))


@dataclass
class ArrowArena:
    arena: np.ndarray          # uint8, the utf8 value bytes (+16 B pad)
    offsets: np.ndarray        # uint64 [n+1], offsets[0] = 0
    labels: np.ndarray         # uint32 Label::Multi indices
    label_offsets: np.ndarray  # uint64 [n+1]

    @property
    def n_records(self):
        return self.offsets.size - 1


def _int_offsets(buf, offset, n, width):
    dt = np.int32 if width == 4 else np.int64
    return np.frombuffer(buf, dt, count=offset + n + 1, offset=0)[offset:offset + n + 1]


def _utf8_column(batch, name):
    """A utf8 column's value bytes (a view of the Arrow buffer, or an empty array), each row's
    start in them and its length (int64; a null row has length 0)."""
    pa = _pa()
    t = batch.column(batch.schema.get_field_index(name))
    if t.type not in (pa.utf8(), pa.large_utf8()):
        raise TypeError(f"{name} must be utf8, got {t.type}")
    n = len(t)
    w = 8 if t.type == pa.large_utf8() else 4
    _, obuf, vbuf = t.buffers()
    o = _int_offsets(obuf, t.offset, n, w).astype(np.int64)
    lens = np.diff(o)
    if t.null_count:
        lens = np.where(np.asarray(t.is_valid()), lens, 0)
    values = np.frombuffer(vbuf, np.uint8) if vbuf is not None and vbuf.size else np.zeros(0, np.uint8)
    return values, o[:-1], lens


_GATHER_BLOCK = 4 << 20  # text bytes a gather step moves: bounds the index temporaries (about 40 B a byte)


def _interleave(cols):
    """Rows of several utf8 columns laid out row by row (A_0 B_0 A_1 B_1 ...), gathered from each
    column's value bytes in place (a sliced batch's buffers are not copied whole): no per-row
    copy, and the index arrays cover at most _GATHER_BLOCK bytes of text at a time (whole rows; a
    longer row goes alone).  -> (body uint8, offsets uint64 [k n + 1])."""
    k, n = len(cols), cols[0][1].size
    lens = np.empty(k * n, np.int64)
    for j, (_, _, ln) in enumerate(cols):
        lens[j::k] = ln
    offs = np.zeros(k * n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    body = np.empty(int(offs[-1]), np.uint8)
    for j, (values, st, ln) in enumerate(cols):
        dst = offs[:-1][j::k]  # where the column's rows go
        cum = np.zeros(n + 1, np.int64)
        np.cumsum(ln, out=cum[1:])
        r0 = 0
        while r0 < n:
            r1 = int(np.searchsorted(cum, cum[r0] + _GATHER_BLOCK, "right")) - 1
            r1 = min(max(r1, r0 + 1), n)
            tot = int(cum[r1] - cum[r0])
            if tot:
                l = ln[r0:r1]
                within = np.arange(tot, dtype=np.int64) - np.repeat(cum[r0:r1] - cum[r0], l)
                body[np.repeat(dst[r0:r1], l) + within] = values[np.repeat(st[r0:r1], l) + within]
            r0 = r1
    return body, offs.astype(np.uint64)


def arena_from_batch(batch, text_col="sentence", label_col="labels", alt_column=None) -> ArrowArena:
    """One record batch -> text arena + offsets + label arrays, read straight
    from the Arrow buffers (nulls are taken as empty text / no labels).
    alt_column: a second utf8 column -- the arena holds the rows of both interleaved (text range
    2r is text_col's row r, range 2r + 1 alt_column's: what the pair calls take), 2n + 1 offsets,
    and the labels stay one set per row."""
    pa = _pa()
    values, starts, lens = _utf8_column(batch, text_col)
    n = lens.size
    if alt_column is not None:
        body, offs = _interleave([(values, starts, lens), _utf8_column(batch, alt_column)])
    elif n and (starts[1:] != starts[:-1] + lens[:-1]).any():  # null rows over non-empty slots
        body, offs = _interleave([(values, starts, lens)])
    else:
        base = int(starts[0]) if n else 0
        end = base + int(lens.sum())
        body = values[base:end]
        offs = np.zeros(n + 1, np.uint64)
        np.cumsum(lens, out=offs[1:])
    arena = np.concatenate([body, np.zeros(16, np.uint8)])

    lc = batch.column(batch.schema.get_field_index(label_col))
    if pa.types.is_integer(lc.type):  # SingleClassArrowGenerator: one label per row, `as u32`
        if lc.null_count:
            raise ValueError("null label")  # Int64Array::value of a null slot is not a label
        vals = (np.asarray(lc, np.int64) & 0xFFFFFFFF).astype(np.uint32)
        return ArrowArena(arena, offs, vals, np.arange(n + 1, dtype=np.uint64))
    if not pa.types.is_list(lc.type) and not pa.types.is_large_list(lc.type):
        raise TypeError(f"{label_col} must be list<int64>, got {lc.type}")
    lo = np.asarray(lc.offsets, dtype=np.int64)
    if lc.null_count:
        valid = np.asarray(lc.is_valid())
        cnt = np.where(valid, np.diff(lo), 0)
        vals = np.concatenate([np.asarray(lc.values[int(s):int(s + c)], np.int64)
                               for s, c in zip(lo[:-1], cnt)] or [np.zeros(0, np.int64)])
        loffs = np.zeros(n + 1, np.uint64)
        np.cumsum(cnt, out=loffs[1:])
    else:
        vals = np.asarray(lc.values, np.int64)[int(lo[0]):int(lo[-1])]
        loffs = (lo - lo[0]).astype(np.uint64)
    if vals.size and (vals.min() < 0 or vals.max() > 0xFFFFFFFF):
        raise ValueError("label index out of u32 range")  # `e.unwrap() as u32` in the reference
    return ArrowArena(arena, offs, vals.astype(np.uint32), loffs)
