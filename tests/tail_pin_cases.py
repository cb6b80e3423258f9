"""Inputs and calls of the token-word pin (tests/test_gpu_tail_pins.py and
tools/gen_tail_pins.py, which records tests/golden/tail_pins.json from this module).

They aim at the 32 KiB level-2 front kernel where a segment with a terminal run writes its token
words per bitmap word ("Run-segment token writer"): thread t makes the words of
positions [32 t, 32 t + 32), a literal word is closed by a match and at the bitmap word's end.
Every input is seeded, at most 64 KiB, and built from random.Random (deflate_pin_cases' helpers);
the path-neighbour stream (neighbour_kinds) repeats two 32 KiB segments of them.

Geometry: match rounds of 2048 positions (a run is proven by the round after the first round
whose last positions all have a candidate, and the whole segment then takes the run path), parse
chunks of 258 bytes, bitmap words of 32 positions, a 4-byte match key.
"""
import hashlib
import random
import zlib

from deflate_pin_cases import period, rnd
from parse_pin_cases import with_repeat

N = 32768
CHUNK = 258
N0 = CHUNK * 24  # random bytes before the run, as parse_pin_cases.literal_skip_run
LEVEL = 2
DICT_LEN = 1024


def run_after(prefix, n=N):
    return prefix + period(251, n - len(prefix))


def word_edges():
    """A 12-byte repeat whose match bit falls on bits 0, 1, 30 and 31 of a bitmap word, and two
    repeats with k literals before a word edge and j after it (the first repeat's 12 bytes end k
    before the edge E, the second starts j after it), all in front of a run."""
    out = {}
    for bit in (0, 1, 30, 31):
        out[f"rep_bit{bit}_run"] = run_after(with_repeat(rnd(N0, 100 + bit), 32 * 40 + bit))
    E = 32 * 50
    for k in (1, 2, 3, 4):
        for j in (1, 2, 3, 4):
            out[f"lit{k}_edge_lit{j}_run"] = run_after(with_repeat(rnd(N0, 110 + 4 * k + j), E - k - 12, E + j))
    return out


def copied_groups(n, group, seed):
    """Groups of one fresh random byte and group - 1 bytes copied from 40 back."""
    r = random.Random(seed)
    b = bytearray(r.randbytes(40))
    while len(b) < n:
        b.append(r.randrange(256))
        for _ in range(group - 1):
            b.append(b[len(b) - 40])
    return bytes(b[:n])


def many_tokens():
    """Thousands of literal words with 32 tokens in most threads, then the run; and prefixes near
    the most words per position: 4-byte groups (the three copied bytes are shorter than the
    4-byte match key: literals, with whatever the candidates make of them) and 5-byte groups
    (literal, match of four, ...: two words per five positions)."""
    return {
        "rnd24576_run": run_after(rnd(24576, 130)),
        "groups4_8192_run": run_after(copied_groups(8192, 4, 131)),
        "groups5_8190_run": run_after(copied_groups(8190, 5, 132)),
        "groups5_20480_run": run_after(copied_groups(20480, 5, 133)),
    }


def ragged_ends():
    """The last bitmap word is partial."""
    out = {f"p251_{CHUNK * k + r}": period(251, CHUNK * k + r) for k in (20, 126) for r in (1, 2, 3, 4, 5)}
    out[f"p251_{N - 3}"] = period(251, N - 3)
    out[f"rnd_run_{N - 3}"] = run_after(rnd(N0, 140), N - 3)
    return out


def sparsest():
    """One token in most bitmap words, none in many."""
    return {"zeros_32768": bytes(N), "p251_32768": period(251, N), "p1_32768": period(1, N)}


GROUPS = {
    "word_edges": word_edges,
    "many_tokens": many_tokens,
    "ragged_ends": ragged_ends,
    "sparsest": sparsest,
}

# the run inputs that also go through the other instantiations of the kernel
OTHERS = ("rep_bit31_run", "lit1_edge_lit3_run", "groups5_8190_run", "p251_32768", "zeros_32768")


def other_inputs():
    made = {}
    for make in GROUPS.values():
        made.update(make())
    return {name: made[name] for name in OTHERS}


def zdict():
    return rnd(DICT_LEN, 150)


def run_free_segment():
    import dmx
    return dmx.corpus("text", N)


def halves_inputs():
    """64 KiB blocks of two 32 KiB halves of which only the second has a run."""
    free = run_free_segment()
    return {f"text_then_{name}": free + data for name, data in other_inputs().items() if len(data) == N}


def neighbour_kinds(G, nseg):
    """Segment i of the path-neighbour stream: workgroup i mod G takes it as its (i // G)-th
    segment, and its segments alternate: a run segment (0) and a run-free one (1)."""
    return [(i % G + i // G) % 2 for i in range(nseg)]


def digest(stream):
    return [len(stream), hashlib.sha256(stream).hexdigest()]


def inflate(comp, zd=None):
    z = zlib.decompressobj(-15, zdict=zd) if zd is not None else zlib.decompressobj(-15)
    out = z.decompress(comp)
    assert z.eof and not z.unused_data
    return out


def batch_streams(ctx, bufs, zd=None):
    """deflate_batch_device at level 2 over 32 KiB buffers placed in turn at a 16-aligned address
    (staged by the early load) and at an odd one."""
    import numpy as np
    import torch
    import dmx
    slot = N + 64
    host = np.zeros(len(bufs) * slot, dtype=np.uint8)
    at = [i * slot + (i % 2) for i in range(len(bufs))]
    for a, b in zip(at, bufs):
        host[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
    arena = torch.from_numpy(host).cuda()
    assert arena.data_ptr() % 16 == 0
    cap = dmx.deflate_bound(N) + 64
    outs = torch.empty(len(bufs) * cap, dtype=torch.uint8, device="cuda")
    kw = {}
    if zd is not None:
        d = torch.frombuffer(bytearray(zd), dtype=torch.uint8).cuda()
        kw = dict(dict_ptr=d.data_ptr(), dict_len=len(zd))
    res = ctx.deflate_batch_device([arena.data_ptr() + a for a in at], [len(b) for b in bufs], LEVEL,
                                   [outs.data_ptr() + i * cap for i in range(len(bufs))], [cap] * len(bufs), **kw)
    torch.cuda.synchronize()
    h = outs.cpu().numpy()
    assert all(status == 0 for _, status, _ in res)
    return [h[i * cap:i * cap + nbytes].tobytes() for i, (nbytes, _, _) in enumerate(res)]


def streams(ctx32, ctx64):
    """{group: {name: (stream, input, dictionary or None)}} of every pinned call."""
    out = {g: {name: (ctx32.compress(data, LEVEL), data, None) for name, data in make().items()}
           for g, make in GROUPS.items()}
    others = other_inputs()
    # every input twice, so each is taken once at the aligned and once at the odd address
    names = list(others) + list(others)[::-1]
    tags = [f"{name}_{'odd' if i % 2 else 'aligned'}" for i, name in enumerate(names)]
    bufs = [others[name] for name in names]
    out["batch"] = {t: (s, b, None) for t, s, b in zip(tags, batch_streams(ctx32, bufs), bufs)}
    zd = zdict()
    out["batch_dict"] = {t: (s, b, zd) for t, s, b in zip(tags, batch_streams(ctx32, bufs, zd), bufs)}
    out["halves"] = {name: (ctx64.compress(data, LEVEL), data, None) for name, data in halves_inputs().items()}
    run, free = others["lit1_edge_lit3_run"], run_free_segment()
    nb = {"run": run, "free": free, "prefix": run + free, "prefix_free_first": free + run}
    out["neighbours"] = {name: (ctx32.compress(data, LEVEL), data, None) for name, data in nb.items()}
    return out
