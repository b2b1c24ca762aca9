"""Pure-Python restatement of StatusWatermarkValve's rules, the reference the valve tests and
the input-channel operator tests compare against.

State: per channel wm = Long.MIN_VALUE, active, aligned; per valve last_wm = Long.MIN_VALUE and
last_status = ACTIVE.  Every input returns the list of what it emitted: ("W", t) and / or
("S", status) with status 0 (active) or -1 (idle), the watermark first."""
LONG_MIN = -(1 << 63)
ACTIVE, IDLE = 0, -1
KIND_WATERMARK, KIND_STATUS = 0, 1


class ReferenceValve:
    def __init__(self, n):
        self.wm = [LONG_MIN] * n
        self.active = [True] * n
        self.aligned = [True] * n
        self.last_wm = LONG_MIN
        self.last_status = ACTIVE

    def _new_min(self, out):
        aligned = [w for w, a in zip(self.wm, self.aligned) if a]
        if aligned and min(aligned) > self.last_wm:
            self.last_wm = min(aligned)
            out.append(("W", self.last_wm))

    def watermark(self, c, t):
        out = []
        if self.last_status != ACTIVE or not self.active[c]:
            return out
        if t <= self.wm[c]:
            return out
        self.wm[c] = t
        if not self.aligned[c] and t >= self.last_wm:
            self.aligned[c] = True
        self._new_min(out)
        return out

    def status(self, c, s):
        if s not in (ACTIVE, IDLE):
            raise ValueError("a watermark status is 0 or -1")
        out = []
        if s == IDLE and self.active[c]:
            self.active[c] = False
            self.aligned[c] = False
            if not any(self.active):
                if self.wm[c] == self.last_wm:
                    top = max(self.wm)
                    if top > self.last_wm:
                        self.last_wm = top
                        out.append(("W", top))
                self.last_status = IDLE
                out.append(("S", IDLE))
            elif self.wm[c] == self.last_wm:
                self._new_min(out)
        elif s == ACTIVE and not self.active[c]:
            self.active[c] = True
            if self.wm[c] >= self.last_wm:
                self.aligned[c] = True
            if self.last_status == IDLE:
                self.last_status = ACTIVE
                out.append(("S", ACTIVE))
        return out

    def event(self, c, kind, value):
        return self.watermark(c, value) if kind == KIND_WATERMARK else self.status(c, value)


def parse_elements(data, vbytes):
    """Python parse of one range's serialized stream elements (4-byte big-endian length, tag,
    body): -> (elements, consumed) with elements a list of ("R", ts or None, value bytes),
    ("W", t), ("S", status) and ("X", tag) for latency markers / record attributes, up to the
    last complete element; consumed = its end."""
    import struct
    out, p, n = [], 0, len(data)
    while p + 4 <= n:
        ln = struct.unpack_from(">i", data, p)[0]
        if ln < 1 or p + 4 + ln > n:
            break
        tag = data[p + 4]
        body = data[p + 5:p + 4 + ln]
        if tag == 0:
            assert ln == 9 + vbytes
            out.append(("R", struct.unpack_from(">q", body, 0)[0], bytes(body[8:])))
        elif tag == 1:
            assert ln == 1 + vbytes
            out.append(("R", None, bytes(body)))
        elif tag == 2:
            assert ln == 9
            out.append(("W", struct.unpack_from(">q", body, 0)[0]))
        elif tag == 6:
            assert ln == 13
            out.append(("W", struct.unpack_from(">q", body, 4)[0]))
        elif tag == 4:
            assert ln == 5
            out.append(("S", struct.unpack_from(">i", body, 0)[0]))
        else:
            out.append(("X", tag))
        p += 4 + ln
    return out, p
