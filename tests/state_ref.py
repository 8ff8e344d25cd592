"""The checkpoint format restated in numpy (include/sph_abi.h "checkpoints"): the checksum with uint64 wrap-around, a blob of the two
mandatory sections assembled from the documented layout, and the damaged blobs every refusal test feeds (with a word of the message each
must produce).  No library call in here."""
import numpy as np

U = np.uint64
MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
LANES = (0x243F6A8885A308D3, 0x13198A2E03707344)
MAGIC = 0x4554415453485053
HEADER_BYTES, ENTRY_BYTES, HEADER_SUMMED = 256, 40, 240
CORE, PARTICLES = 1, 2


def _mix64(z):
    z = z ^ (z >> U(30))
    z = z * U(0xBF58476D1CE4E5B9)
    z = z ^ (z >> U(27))
    z = z * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def checksum(buf, base=0):
    """(lo, hi) of a buffer of a multiple of 8 bytes, word index `base` at its first word."""
    raw = np.frombuffer(bytes(buf) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).tobytes(), np.uint8)
    assert raw.size % 8 == 0
    w = raw.view("<u8").astype(U)
    with np.errstate(over="ignore"):
        k = w + (U(base) + np.arange(len(w), dtype=U)) * U(G)
        return tuple(int(_mix64(k + U(c)).sum(dtype=U)) for c in LANES)


def add(a, b):
    return tuple((x + y) & MASK for x, y in zip(a, b))


def align16(v):
    return (v + 15) & ~15


def core_payload(pkg, params, last_dt=0.0):
    """The core section of an engine that has not dispatched yet: params, lastDt, default fountain and river, no heightfield, no targets."""
    import ctypes as C
    c = pkg.SphStateCore()
    C.memmove(C.byref(c.params), C.byref(params), C.sizeof(pkg.SphParams))
    c.lastDt = last_dt
    pkg.load_library().sph_fountain_default(C.byref(c.fountain))
    pkg.load_library().sph_river_default(C.byref(c.river))
    return bytes(c)


def assemble(params_bytes, n, sections, fmt=1, abi=4, kind=1):
    """A blob from (tag, payload bytes) pairs in the given order, laid out and summed as the format says."""
    count = len(sections)
    at = HEADER_BYTES + ENTRY_BYTES * count
    table, body = b"", b""
    mask = 0
    for tag, payload in sections:
        start = align16(at)
        body += b"\0" * (start - at) + payload
        lo, hi = checksum(payload)
        table += np.array([tag, 1], "<u4").tobytes() + np.array([start, len(payload), lo, hi], "<u8").tobytes()
        at = start + len(payload)
        mask |= tag
    total = align16(at)
    body += b"\0" * (total - at)
    head = np.array([MAGIC], "<u8").tobytes() + np.array([fmt, abi, kind, count], "<u4").tobytes() + np.array([n, total], "<u8").tobytes() + \
        np.array([mask, HEADER_BYTES], "<u4").tobytes() + params_bytes
    head += b"\0" * (HEADER_SUMMED - len(head))
    lo, hi = add(checksum(head), checksum(table, HEADER_SUMMED // 8))
    return np.frombuffer(head + np.array([lo, hi], "<u8").tobytes() + table + body, np.uint8).copy()


def build_blob(pkg, records, params, **kw):
    """A core + particles blob of `records` under `params`."""
    return assemble(bytes(params), len(records), [(CORE, core_payload(pkg, params)), (PARTICLES, records.tobytes())], **kw)


def reseal(blob):
    """The header checksum recomputed after an edit of the header or the table (so that the edit itself is what gets refused)."""
    b = blob.copy()
    count = int(b[20:24].view("<u4")[0])
    table = b[HEADER_BYTES:HEADER_BYTES + ENTRY_BYTES * count].tobytes()
    b[HEADER_SUMMED:HEADER_BYTES] = np.frombuffer(np.array(add(checksum(b[:HEADER_SUMMED]), checksum(table, HEADER_SUMMED // 8)), "<u8").tobytes(), np.uint8)
    return b


def _entry_field(blob, index, field, value):
    """Entry `index` of the table with its offset (field 0) or bytes (field 1) replaced, resealed."""
    b = blob.copy()
    at = HEADER_BYTES + ENTRY_BYTES * index + 8 + 8 * field
    b[at:at + 8] = np.frombuffer(np.array([value], "<u8").tobytes(), np.uint8)
    return reseal(b)


def damaged_blobs(pkg, records, params):
    """(name, blob, a word its refusal must contain) for every damage the issue lists."""
    good = build_blob(pkg, records, params)
    info = pkg.state_sections(good)
    core, part = info["sections"]["core"], info["sections"]["particles"]
    out = [("truncated", good[:len(good) - 16].copy(), "truncated"),
           ("cut inside the header", good[:100].copy(), "truncated")]
    b = good.copy()
    b[0] ^= 0xFF
    out.append(("wrong magic", b, "magic"))
    out.append(("future format version", build_blob(pkg, records, params, fmt=2), "format version"))
    out.append(("section past the end", _entry_field(good, 1, 1, part["bytes"] + 4096), "past the end"))
    out.append(("overlapping sections", _entry_field(good, 1, 0, core["offset"] + 16), "overlaps"))
    b = good.copy()
    b[part["offset"] + 41] ^= 0x10
    out.append(("wrong checksum", b, "checksum"))
    out.append(("unknown tag", assemble(bytes(params), len(records), [(CORE, core_payload(pkg, params)), (PARTICLES, records.tobytes()), (1 << 9, b"\0" * 16)]),
                "unknown section tag"))
    out.append(("n = 0", build_blob(pkg, records[:0], params), "n = 0"))
    return good, out
