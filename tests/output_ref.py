"""NumPy restatement of the device-side output (include/csi.h, csi_output_*): record layout, ownership, masking, conversion,
accumulation order and division -- and a stand-in recorder with the methods of climaseaice.jl_amd.output.DeviceRecorder, so that
schedules, weights and files are tested without a device.

Everything here works on PARENT arrays (halos included), as Field.numpy() returns them: shape (nj, ni), element (i, j) (1-based) at
[j + Hy - 1, i + Hx - 1]."""
import numpy as np

ALIGN = 256


def interior(parent, Hx, Hy):
    """The field's OWN interior: the parent minus its halos -- (Ny, Nx), one more column / row for a Face field on a Bounded high side
    (the parent is that much larger).  On a tile only the easternmost / northernmost tile's parent has the extra face."""
    nj, ni = parent.shape
    return parent[Hy:nj - Hy, Hx:ni - Hx]


def layout(shapes, dtypes):
    """Byte offset of every field of a record and the record's size: fields in list order, each a dense row-major (ny, nx) array of 4-
    ("f32") or 8-byte ("f64") elements, each starting at a multiple of 256; the record ends on one as well."""
    at, offs = 0, []
    for (ny, nx), d in zip(shapes, dtypes):
        offs.append(at)
        at += ny * nx * (4 if d == "f32" else 8)
        at = -(-at // ALIGN) * ALIGN
    return offs, at


def convert(x, dtype):
    """fp32 output: NumPy's astype(float32) -- round to nearest even, overflow to +-Inf, subnormal results kept."""
    if dtype == "f64":
        return np.array(x, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


def accumulate(acc, x, w):
    """acc = acc + (x * w): the product is rounded first (no fused multiply-add)."""
    with np.errstate(all="ignore"):
        p = x * np.float64(w)
        return acc + p


def total_weight(weights):
    W = 0.0
    for w in weights:
        W = W + float(w)
    return W


def average(acc, W):
    with np.errstate(all="ignore"):
        return acc / np.float64(W)


def element(x, dtype, mask=None, fill=np.nan):
    """A record field from its values x (a snapshot's interior or an average): fill in inactive cells (mask == 0), then the conversion."""
    x = np.array(x, dtype=np.float64)
    if mask is not None:
        x = np.where(mask != 0, x, np.float64(fill))
    return convert(x, dtype)


def averaged(interiors, weights):
    """acc / W of a window: acc from +0.0 in the order of the calls, W summed on the host in the same order."""
    acc = np.zeros_like(np.asarray(interiors[0], dtype=np.float64))
    for x, w in zip(interiors, weights):
        acc = accumulate(acc, np.asarray(x, dtype=np.float64), w)
    return average(acc, total_weight(weights))


def same_bits(a, b):
    """Bit for bit, NaN equal to NaN (payloads are not specified)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))).all())


def split_record(record, shapes, dtypes):
    """The fields of a packed record (uint8 array) as arrays."""
    offs, total = layout(shapes, dtypes)
    assert len(record) == total, (len(record), total)
    out = []
    for off, (ny, nx), d in zip(offs, shapes, dtypes):
        t = np.float32 if d == "f32" else np.float64
        out.append(record[off:off + ny * nx * np.dtype(t).itemsize].view(t).reshape(ny, nx))
    return out


class RefRecorder:
    """Stand-in for output.DeviceRecorder on a model-like object with .grid, .fields (name -> Field on the CPU) and optionally
    .mask_interior ((Ny, Nx) bytes): the same slot rules, the arithmetic above."""

    @staticmethod
    def bound_fields(model):
        return {n: (f, n) for n, f in model.fields.items()}

    def __init__(self, model, specs, slots):
        self.model, self.specs, self.nslots = model, list(specs), int(slots)
        g = model.grid
        self.H = (g.Hx, g.Hy)
        self.shapes = [interior(model.fields[s].numpy(), *self.H).shape for s, *_ in specs]
        self.dtypes = [d for _, d, *_ in specs]
        offs, self.record_bytes = layout(self.shapes, self.dtypes)
        self.layout = [(o, ny, nx) for o, (ny, nx) in zip(offs, self.shapes)]
        self.acc = [np.zeros(s) for s in self.shapes]
        self.W = 0.0
        self.slot = [None] * self.nslots
        self.snapshots = 0

    def _x(self, k):
        return interior(self.model.fields[self.specs[k][0]].numpy(), *self.H).copy()

    def accumulate(self, w):
        assert w > 0 and np.isfinite(w)
        for k, spec in enumerate(self.specs):
            if spec[2]:
                self.acc[k] = accumulate(self.acc[k], self._x(k), w)
        self.W = self.W + w

    def snapshot(self):
        any_avg = any(s[2] for s in self.specs)
        if any_avg and self.W == 0.0:
            raise ValueError("W == 0")
        free = [q for q in range(self.nslots) if self.slot[q] is None]
        if not free:
            raise ValueError("no free slot")
        rec = np.zeros(self.record_bytes, dtype=np.uint8)
        mask = getattr(self.model, "mask_interior", None)
        for k, (name, d, avg, masked, fill) in enumerate(self.specs):
            x = average(self.acc[k], self.W) if avg else self._x(k)
            a = element(x, d, mask if masked else None, fill)
            off = self.layout[k][0]
            rec[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
            if avg:
                self.acc[k] = np.zeros(self.shapes[k])
        self.W = 0.0
        self.slot[free[0]] = rec
        self.snapshots += 1
        return free[0]

    def wait(self, slot):
        assert self.slot[slot] is not None, "slot not in flight"
        return self.slot[slot]

    def release(self, slot):
        assert self.slot[slot] is not None, "slot not in flight"
        self.slot[slot] = None

    def close(self):
        assert all(s is None for s in self.slot), "closed with records in flight"
