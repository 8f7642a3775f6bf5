"""Footprint checks: which elements of its buffers a device entry writes, and reads.

No GPU code here.  An ``Arena`` carves every input and output of one call out of one byte
buffer filled with a single byte value; the call runs twice, on arenas filled with 0xA5 and
0x5A, and ``check_writes`` compares the two results with the mask of elements include/x264hip.h
says the entry writes:

* outside the mask every byte still holds what it held before the call, in both runs;
* inside the mask the two runs agree -- an element the entry failed to write keeps two
  different fills, and a result that depends on a guard byte the entry should not have read
  differs too.

The guards are large on purpose (4096 bytes around lists and tables; 16 rows above and below
every frame of a plane, 3 more rows between frames, 64 pixels of stride slack), so an overrun of
a few rows or items stays inside a live allocation and is reported, not faulted on.  The same
arena serves numpy (the oracle, tests/test_cpu_footprint.py) and torch (the HIP entries,
tests/test_gpu_footprint.py): buffers are byte offsets, ``Buf.np`` / ``Buf.t`` view them.

The mask functions at the end quote the header sentence they encode.
"""
import numpy as np

FILLS = (0xA5, 0x5A)
PAD = 32


class Geometry:
    """guard sizes of an arena"""

    def __init__(self, guard_bytes=4096, guard_rows=16, gap_rows=3, slack=64):
        self.guard_bytes, self.guard_rows, self.gap_rows, self.slack = guard_bytes, guard_rows, gap_rows, slack


GUARDED = Geometry()
# the wrappers' own allocation: no guards, frames back to back, plane_stride() rows
TIGHT = Geometry(0, 0, 0, 0)


def plane_stride(width, pad=PAD):
    return (width + 2 * pad + 63) // 64 * 64


def fill_value(dtype, fill):
    return np.frombuffer(bytes([fill]) * np.dtype(dtype).itemsize, dtype)[0]


def _torch_dtype(dtype):
    import torch
    return {"uint8": torch.uint8, "int8": torch.int8, "int16": torch.int16, "uint16": torch.int16,
            "int32": torch.int32, "uint32": torch.int32, "int64": torch.int64, "uint64": torch.int64,
            "float32": torch.float32}[np.dtype(dtype).name]


class Buf:
    """`nbytes` of the arena at byte `start`: guards included.  `shape` is the shape of the whole
    region in elements of `dtype` (``np`` / ``t`` view it), `coords` maps an index of that shape to
    the coordinates a message names."""

    def np(self, host):
        return host[self.start:self.start + self.nbytes].view(self.dtype).reshape(self.shape)

    def t(self, dev):
        return dev[self.start:self.start + self.nbytes].view(_torch_dtype(self.dtype)).view(self.shape)

    def none(self):
        return np.zeros(self.shape, bool)


class ListBuf(Buf):
    """[items, fields...] elements with `guard` elements of fill before and after; the payload
    is ``data(host)`` / ``dt(dev)``.  Coordinates: (item, field), item < 0 or >= items in a guard."""
    labels = ("item", "field")

    def __init__(self, name, start, shape, dtype, guard_bytes):
        self.name, self.start, self.dtype = name, start, np.dtype(dtype)
        self.pshape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.n = int(np.prod(self.pshape))
        self.guard = guard_bytes // self.dtype.itemsize
        self.shape = (self.n + 2 * self.guard,)
        self.nbytes = self.shape[0] * self.dtype.itemsize
        self.fields = max(1, self.n // max(1, self.pshape[0])) if self.pshape else 1

    def data(self, host):
        return self.np(host)[self.guard:self.guard + self.n].reshape(self.pshape)

    def dt(self, dev):
        return self.t(dev)[self.guard:self.guard + self.n].view(self.pshape)

    def mask(self, payload_mask=True):
        """the whole-region mask of a payload mask (True: the whole payload)"""
        m = self.none()
        m[self.guard:self.guard + self.n] = np.broadcast_to(np.asarray(payload_mask, bool), self.pshape).ravel()
        return m

    def items(self, n_items):
        """items [0, n_items) written, the rest of the payload not"""
        pm = np.zeros(self.pshape, bool)
        pm[:n_items] = True
        return self.mask(pm)

    def coords(self, idx):
        e = int(idx[0]) - self.guard
        return (e // self.fields, e % self.fields)


class PlaneBuf(Buf):
    """`nframes` padded planes of a width x height picture, pixel (0,0) of frame 0 at element
    `origin`, `pad_x` / `pad_y` pixels of padding the reference may read, rows `stride` apart,
    frames `frame_stride` apart.  Each frame: guard rows, pad_y + height + pad_y rows, guard rows,
    gap rows.  Coordinates: (frame, row, col) of the picture; a column >= width + pad_x is stride
    slack, a row < -pad_y or >= height + pad_y a guard row or the inter-frame gap."""
    labels = ("frame", "row", "col")

    def __init__(self, name, start, nframes, width, height, dtype, geom, pad_x=PAD, pad_y=PAD, extra=0,
                 stride=None, rows=None):
        self.name, self.start, self.dtype = name, start, np.dtype(dtype)
        self.nframes, self.width, self.height, self.pad_x, self.pad_y = nframes, width, height, pad_x, pad_y
        self.guard_rows = geom.guard_rows
        self.stride = stride if stride is not None else plane_stride(width, pad_x) + geom.slack + (extra if geom.slack else 0)
        self.rows = rows if rows is not None else height + 2 * pad_y      # rows the entry may touch
        self.frame_rows = self.rows + 2 * geom.guard_rows + geom.gap_rows
        self.frame_stride = self.frame_rows * self.stride
        self.origin = (geom.guard_rows + pad_y) * self.stride + pad_x
        self.shape = (nframes, self.frame_rows, self.stride)
        self.nbytes = nframes * self.frame_stride * self.dtype.itemsize

    def picture(self, host):
        """the padded pictures [nframes, rows, width + 2 * pad_x]: what the reference may read"""
        g = self.guard_rows
        return self.np(host)[:, g:g + self.rows, :self.width + 2 * self.pad_x]

    def rect(self, x0, x1, y0, y1):
        """mask of columns [x0, x1) x rows [y0, y1) (picture coordinates) of every frame"""
        m = self.none()
        r, c = self.guard_rows + self.pad_y, self.pad_x
        assert 0 <= c + x0 <= c + x1 <= self.stride and 0 <= r + y0 <= r + y1 <= self.frame_rows
        m[:, r + y0:r + y1, c + x0:c + x1] = True
        return m

    def body(self, dev):
        """torch view [nframes, rows, stride] from the first padding row on (frame stride kept)"""
        g = self.guard_rows
        return self.t(dev)[:, g:g + self.rows]

    def coords(self, idx):
        f, r, c = (int(v) for v in idx)
        return (f, r - self.guard_rows - self.pad_y, c - self.pad_x)


class Arena:
    """one byte buffer filled with `fill`, carved front to back"""

    def __init__(self, fill, geom=GUARDED, capacity=2 << 20):
        self.fill, self.geom = fill, geom
        self.host = np.full(capacity, fill, np.uint8)
        self.used = 0
        self.bufs = []

    def _grow(self, need):
        if need > self.host.size:               # (buffers are offsets: views are made on demand)
            self.host = np.concatenate([self.host, np.full(max(need, 2 * self.host.size) - self.host.size,
                                                           self.fill, np.uint8)])

    def _take(self, buf):
        self._grow(buf.start + buf.nbytes + self.geom.guard_bytes)
        self.used = buf.start + buf.nbytes
        self.bufs.append(buf)
        return buf

    def _start(self):
        return (self.used + 4095) // 4096 * 4096       # keeps every alignment the ABI asks for

    def list(self, name, shape, dtype, data=None, valid=None):
        """`data` fills the payload; `valid` = n says the caller stores items [0, n) itself and the
        entry may read only those (the items after stay fill).  `readable` marks what may be read."""
        b = self._take(ListBuf(name, self._start(), shape, dtype, self.geom.guard_bytes))
        b.readable = b.items(valid) if valid is not None else b.mask(data is not None)
        if data is not None:
            a = np.ascontiguousarray(data)
            if a.dtype != b.dtype and a.dtype.kind in "iu" and a.dtype.itemsize == b.dtype.itemsize:
                a = a.view(b.dtype)                      # uint16 bit patterns in an int16 buffer
            b.data(self.host)[...] = a.reshape(b.pshape)
        return b

    def plane(self, name, nframes, width, height, dtype, data=None, **kw):
        start = self._start()
        if self.geom.guard_bytes:
            start += self.geom.guard_bytes
        b = self._take(PlaneBuf(name, start, nframes, width, height, dtype, self.geom, **kw))
        self.used += self.geom.guard_bytes
        b.readable = b.none()
        if data is not None:
            b.picture(self.host)[...] = data
            g = b.guard_rows
            b.readable[:, g:g + b.rows, :b.width + 2 * b.pad_x] = True
        return b

    def bytes(self):
        return self.host[:self.used]

    def device(self):
        import torch
        return torch.from_numpy(self.bytes().copy()).cuda()


def _first(buf, where, k=4):
    idx = np.argwhere(where)[:k]
    return [buf.coords(i) for i in idx], int(where.sum())


def check_writes(run1, run2, mask, buf, maybe=None, fills=FILLS):
    """run1 / run2: `buf`'s whole region after the call on the arenas filled with fills[0] /
    fills[1], or (before, after) pairs when the region held data (in-place entries, inputs).
    mask: True where the header says the entry writes.  maybe: elements the header leaves to
    the data (either is fine).  Raises AssertionError naming the first offending coordinates."""
    mask = np.asarray(mask, bool)
    free = np.zeros_like(mask) if maybe is None else np.asarray(maybe, bool)
    after = []
    for run, fill in zip((run1, run2), fills):
        before, aft = run if isinstance(run, tuple) else (fill_value(buf.dtype, fill), run)
        assert aft.shape == mask.shape, (buf.name, aft.shape, mask.shape)
        bad = (aft != before) & ~mask & ~free
        if bad.any():
            at, n = _first(buf, bad)
            raise AssertionError("%s: %d element(s) written outside the footprint (fill 0x%02X), first at %s %s"
                                 % (buf.name, n, fill, buf.labels, at))
        after.append(aft)
    diff = (after[0] != after[1]) & mask & ~free
    if diff.any():
        at, n = _first(buf, diff)
        raise AssertionError("%s: %d footprint element(s) not written, or dependent on guard bytes: the two "
                             "runs disagree, first at %s %s" % (buf.name, n, buf.labels, at))


def written(run1, run2, buf, fills=FILLS):
    """elements either run changed (a value equal to one fill differs from the other)"""
    return (run1 != fill_value(buf.dtype, fills[0])) | (run2 != fill_value(buf.dtype, fills[1]))


def check_arena(ar1, after1, ar2, after2, outputs, maybe=None):
    """check_writes over every buffer of two arenas carved alike: `outputs` {buf name: mask};
    every other buffer (the inputs) must come back unchanged.  after*: the arenas' bytes after
    the call; the arenas still hold the bytes before it."""
    maybe = maybe or {}
    assert [b.name for b in ar1.bufs] == [b.name for b in ar2.bufs] and ar1.used == ar2.used
    assert set(outputs) <= {b.name for b in ar1.bufs}, "unknown output"
    covered = np.zeros(ar1.used, bool)
    for b in ar1.bufs:
        covered[b.start:b.start + b.nbytes] = True
        check_writes((b.np(ar1.bytes()), b.np(after1)), (b.np(ar2.bytes()), b.np(after2)),
                     outputs.get(b.name, b.none()), b, maybe.get(b.name))
    for ar, aft in ((ar1, after1), (ar2, after2)):
        bad = (aft != ar.bytes()) & ~covered
        assert not bad.any(), "bytes between the buffers written, first at arena offset %d" % np.argmax(bad)


# ------------------------------------------------------------------ footprint masks (include/x264hip.h)
def hpel_mask(buf):
    """hpel_filter: "writes the H, V and centre planes over [-32, width+32) x [-32, height+32)" """
    return buf.rect(-32, buf.width + 32, -32, buf.height + 32)


def lowres_mask(buf):
    """frame_init_lowres: "the four half-resolution planes dst[0..3] (full-pel, H, V, centre) over
    [-32, width/2+32) x [-32, height/2+32)" -- buf is one lowres plane (its width = width/2)"""
    return buf.rect(-32, buf.width + 32, -32, buf.height + 32)


def weight_scale_cols(width):
    """weight_scale_plane: "the reference weights 16-wide strips while x < width-8 and one 8-wide
    strip after, so up to 7 columns past width are written too" -> columns [0, this)"""
    x = 0
    while x < width - 8:
        x += 16
    return x + 8 if x < width else x


def weight_scale_mask(buf, x0, y0, width, height):
    """weight_scale_plane: "dst = mc_weight(src) over the width x height region at the pointers"
    (the pointers at picture (x0, y0)) plus the strip rounding of weight_scale_cols; the same
    columns of src are read"""
    return buf.rect(x0, x0 + weight_scale_cols(width), y0, y0 + height)


def integral_masks(buf, lines, padh, sub8x8):
    """frame_integral: "Writes the 8x8 box sums of rows [1-32, lines+32-8) and columns [-padh,
    stride-padh-8) ... and, when sub8x8, the 4x4 box sums in the second plane at
    +stride*(lines+64)" over the same rows and columns.  buf: the integral buffer, its rows =
    (2 if sub8x8 else 1) * (lines + 64), pad_x = padh.  Returns (mask, scratch): scratch = what
    the reference function uses as working storage in the 8x8 plane and the HIP entry leaves
    alone -- its zeroed row -32, the horizontal sums of its last 8 rows [lines+24, lines+32)
    (whole strides both) and, when sub8x8, columns [stride-padh-8, stride-padh-4) of every row,
    which its 4-wide horizontal sums reach."""
    m, s = buf.none(), buf.none()
    g = buf.guard_rows
    m[:, g + 1:g + lines + 56, 0:buf.stride - 8] = True
    s[:, g, :] = True
    s[:, g + lines + 56:g + lines + 64, :] = True
    if sub8x8:
        h = lines + 64
        m[:, g + h + 1:g + h + lines + 56, 0:buf.stride - 8] = True
        s[:, g + 1:g + h, buf.stride - 8:buf.stride - 4] = True
    return m, s & ~m


def recon_mask(buf, mb_width, mb_height):
    """mb_dequant_idct_add: "recon = clip( pred + idct( dequant( dct ) ) ) per MB": exactly the
    16*mb_width x 16*mb_height rectangle of each frame"""
    return buf.rect(0, 16 * mb_width, 0, 16 * mb_height)


def table_mask(buf):
    """me_search_full / me_search_full8 / me_search_centred: "row pitch P = (2*range+1 + 3) & ~3
    (entries i > 2*range are padding, and every one is written ...).  The call writes exactly the
    n_frames*mb_height*mb_width*(2*range+1)*P entries": the whole table, padding entries included
    -- the oracle's tables have no padding -- and nothing after the last macroblock's last row"""
    return buf.mask(True)


def blocks_mask(buf, offs, bw, bh, stride):
    """block lists (add_idct_batch "on dst + dst_off[i] (stride dst_stride)", zigzag_sub_batch
    "dst block is overwritten with the src block"): the bw x bh block at each element offset of
    the payload"""
    pm = np.zeros(buf.n, bool)
    for o in np.asarray(offs).tolist():
        for y in range(bh):
            pm[o + y * stride:o + y * stride + bw] = True
    return buf.mask(pm.reshape(buf.pshape))
