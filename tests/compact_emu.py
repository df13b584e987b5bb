"""The compact result form in plain Python, written from the text of include/pgx.h ("compact result") alone: what the device encoder
(pgx_batch_result_compact, pgx_compact_encode) must produce byte for byte, and what pgx_compact_expand must read.

A result is the dict Batch.result() returns: mem_offsets uint64[n_reads + 1], mems (start, end, bwt_start, size), and for the tagged
form tag_run_counts uint64[n_mems], pos_offsets uint64[n_mems + 1], positions.  The compact form is the dict Batch.result_compact()
returns: counters, block_offsets / block_first_mem / block_first_pos uint64[n_blocks + 1], bytes uint8[n_bytes]."""
import numpy as np

BLOCK_READS = 64
TAGS = 1
M64 = (1 << 64) - 1


def varint(v):
    """unsigned LEB128, shortest form: seven bits a byte, low bits first, high bit = another byte follows"""
    v = int(v) & M64
    out = bytearray()
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def read_varint(buf, i, end):
    """(value, next index) of the varint at buf[i]; ValueError where the header says PGX_ERR_FORMAT"""
    v = 0
    for k in range(10):
        if i >= end:
            raise ValueError("truncated")
        c = buf[i]
        i += 1
        if k == 9 and c > 1:
            raise ValueError("varint longer than 10 bytes" if c & 0x80 else "tenth byte above 1")
        v |= (c & 0x7F) << (7 * k)
        if not c & 0x80:
            return v, i
    raise ValueError("varint longer than 10 bytes")


def encode_block(res, k, tags):
    mo = res["mem_offsets"]
    n = len(mo) - 1
    r0, r1 = BLOCK_READS * k, min(BLOCK_READS * k + BLOCK_READS, n)
    m0, m1 = int(mo[r0]), int(mo[r1])
    out = bytearray()
    for r in range(r0, r1):
        out += varint(int(mo[r + 1]) - int(mo[r]))
    mems = res["mems"]
    for m in range(m0, m1):
        start, end = int(mems["start"][m]), int(mems["end"][m])
        out += varint(start) + varint(end - start) + varint(int(mems["bwt_start"][m])) + varint(int(mems["size"][m]))
        if tags:
            out += varint(int(res["tag_run_counts"][m])) + varint(int(res["pos_offsets"][m + 1]) - int(res["pos_offsets"][m]))
    if tags:
        po, pos = res["pos_offsets"], res["positions"]
        for m in range(m0, m1):
            prev = 0
            for i in range(int(po[m]), int(po[m + 1])):
                out += varint(int(pos[i]) - prev)  # (the first as it is; mod 2^64)
                prev = int(pos[i])
    out += bytes(-len(out) % 8)
    return bytes(out)


def encode(res):
    """result dict -> compact dict (tagged exactly when the result has pos_offsets)"""
    tags = "pos_offsets" in res
    mo = res["mem_offsets"]
    n, m = len(mo) - 1, len(res["mems"])
    nb = (n + BLOCK_READS - 1) // BLOCK_READS
    blocks = [encode_block(res, k, tags) for k in range(nb)]
    offs = np.zeros(nb + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(b) for b in blocks], dtype=np.uint64)
    first_mem = np.array([int(mo[min(BLOCK_READS * k, n)]) for k in range(nb + 1)], dtype=np.uint64)
    first_pos = np.array([int(res["pos_offsets"][int(x)]) if tags else 0 for x in first_mem], dtype=np.uint64)
    stream = np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()
    return dict(n_reads=n, n_mems=m, n_positions=len(res["positions"]) if tags else 0, n_extensions=int(res.get("n_extensions", 0)),
                n_tag_overflow=int(res.get("n_tag_overflow", 0)), flags=TAGS if tags else 0, block_reads=BLOCK_READS, n_blocks=nb,
                n_bytes=len(stream), block_offsets=offs, block_first_mem=first_mem, block_first_pos=first_pos, bytes=stream, ms_encode=0.0)


def decode(c):
    """compact dict -> (mem_offsets, mems as uint64[n_mems, 4], tag_run_counts, pos_offsets, positions); the last three None without tags"""
    tags = bool(c["flags"] & TAGS)
    n, m = c["n_reads"], c["n_mems"]
    buf = bytes(c["bytes"])
    mo = np.zeros(n + 1, dtype=np.uint64)
    mems = np.zeros((m, 4), dtype=np.uint64)
    runs = np.zeros(m, dtype=np.uint64) if tags else None
    po = np.zeros(m + 1, dtype=np.uint64) if tags else None
    pos = np.zeros(c["n_positions"], dtype=np.uint64) if tags else None
    for k in range(c["n_blocks"]):
        i, end = int(c["block_offsets"][k]), int(c["block_offsets"][k + 1])
        r0, r1 = BLOCK_READS * k, min(BLOCK_READS * k + BLOCK_READS, n)
        mi = int(c["block_first_mem"][k])
        m0 = mi
        for r in range(r0, r1):
            cnt, i = read_varint(buf, i, end)
            mo[r] = mi
            mi += cnt
        assert mi == int(c["block_first_mem"][k + 1])
        pi = int(c["block_first_pos"][k])
        counts = []
        for x in range(m0, mi):
            f = []
            for _ in range(6 if tags else 4):
                v, i = read_varint(buf, i, end)
                f.append(v)
            mems[x] = (f[0], (f[0] + f[1]) & M64, f[2], f[3])
            if tags:
                runs[x] = f[4]
                po[x] = pi
                pi += f[5]
                counts.append(f[5])
        if tags:
            assert pi == int(c["block_first_pos"][k + 1])
            for x, cnt in zip(range(m0, mi), counts):
                v = 0
                for j in range(cnt):
                    d, i = read_varint(buf, i, end)
                    v = (v + d) & M64
                    pos[int(po[x]) + j] = v
        assert end - i < 8 and not any(buf[i:end])
    mo[n] = m
    if tags:
        po[m] = c["n_positions"]
    return mo, mems, runs, po, pos


def random_result(rng, n_reads, tags, max_mems=4, max_pos=5, p_empty=0.3, big=False):
    """a random result dict: reads with 0 .. max_mems MEMs (p_empty of them with none), MEMs with 0 .. max_pos positions; big: values over the
    whole 64-bit range in place of realistic ones"""
    from pgx_ffi import MEM_DTYPE

    cnt = rng.integers(0, max_mems + 1, n_reads)
    cnt[rng.random(n_reads) < p_empty] = 0
    mo = np.zeros(n_reads + 1, dtype=np.uint64)
    mo[1:] = np.cumsum(cnt)
    m = int(mo[-1])

    def vals(k, hi):
        if big:
            return (rng.integers(0, 1 << 63, k, dtype=np.uint64) << np.uint64(1)) >> rng.integers(0, 64, k).astype(np.uint64)
        return rng.integers(0, hi, k, dtype=np.uint64)

    mems = np.zeros(m, dtype=MEM_DTYPE)
    mems["start"] = vals(m, 150)
    mems["end"] = mems["start"] + vals(m, 150)
    mems["bwt_start"] = vals(m, 1 << 33)
    mems["size"] = vals(m, 300).astype(np.int64)
    res = dict(mem_offsets=mo, mems=mems, n_extensions=int(rng.integers(0, 1000)), n_tag_overflow=0)
    if tags:
        pc = rng.integers(0, max_pos + 1, m)
        po = np.zeros(m + 1, dtype=np.uint64)
        po[1:] = np.cumsum(pc)
        pos = vals(int(po[-1]), 1 << 40)
        if not big:  # ascending within a MEM, as real results are
            for x in range(m):
                pos[int(po[x]):int(po[x + 1])].sort()
        res.update(tag_run_counts=vals(m, 40), pos_offsets=po, positions=pos)
    return res


def border_values():
    """2^(7j) - 1 and 2^(7j) for every j up to 9 (where a varint grows by a byte), and 2^64 - 1"""
    out = []
    for j in range(10):
        out += [max((1 << (7 * j)) - 1, 0), 1 << (7 * j)]
    return sorted(set(out + [M64]))


def border_result(tags=True):
    """every border value (2^(7j) - 1, 2^(7j), 2^64 - 1) in every field: start, end - start, bwt_start, size, run count, position count (up to
    2^14), first position, difference; one MEM a read, so the values spread over several blocks"""
    from pgx_ffi import MEM_DTYPE

    b = np.array(border_values(), dtype=np.uint64)
    n = len(b)
    mems = np.zeros(4 * n, dtype=MEM_DTYPE)
    mems["start"][:n] = b
    mems["end"][:n] = b  # (length 0)
    mems["end"][n:2 * n] = b  # start 0: end - start = b
    mems["bwt_start"][2 * n:3 * n] = b
    mems["size"][3 * n:] = b.astype(np.int64)  # (2^63 and beyond: negative sizes)
    res = dict(mem_offsets=np.arange(4 * n + 1, dtype=np.uint64), mems=mems)
    if tags:
        runs = np.zeros(4 * n, dtype=np.uint64)
        runs[:n] = b
        pc = np.zeros(4 * n, dtype=np.int64)
        pc[n:2 * n] = 2  # first position b, then b + b: the difference is b again
        small = [int(v) for v in b if v <= 1 << 14]
        pc[2 * n:2 * n + len(small)] = small  # position counts at the borders
        po = np.concatenate([[0], np.cumsum(pc)]).astype(np.uint64)
        pos = np.zeros(int(po[-1]), dtype=np.uint64)
        pos[po[n:2 * n].astype(np.int64)] = b
        pos[po[n:2 * n].astype(np.int64) + 1] = b + b  # (wraps)
        for i in range(len(small)):
            pos[int(po[2 * n + i]):int(po[2 * n + i + 1])] = np.arange(small[i], dtype=np.uint64) * np.uint64(3)
        res.update(tag_run_counts=runs, pos_offsets=po, positions=pos)
    return res


def same_result(a, b):
    """the arrays of two result dicts are equal (counters aside)"""
    keys = ["mem_offsets", "mems"] + (["tag_run_counts", "pos_offsets", "positions"] if "pos_offsets" in a else [])
    return ("pos_offsets" in a) == ("pos_offsets" in b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def same_compact(a, b):
    """two compact dicts hold the same stream and tables (ms_encode and the run counters aside)"""
    if any(int(a[k]) != int(b[k]) for k in ("n_reads", "n_mems", "n_positions", "flags", "block_reads", "n_blocks", "n_bytes")):
        return False
    return all(np.array_equal(a[k], b[k]) for k in ("block_offsets", "block_first_mem", "block_first_pos", "bytes"))
