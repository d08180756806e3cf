"""Generate the execution-plan fixtures used by the executor tests.

The plans use the reference's JSON plan format (the one its DSL emits and
src/core/executor/execution_plan.cc parses); this script is this repo's own generator of three
AllReduce algorithms over memory channels:

  allreduce_pkt_n{N}.json    LL protocol, all-pairs: ppkt every peer's chunk into its scratch,
                             respkt my chunk (sum of the peers' packets + mine, sent back as
                             packets), upkt the other chunks; T threadblocks split every chunk
                             with tbg_info.  Same operation mix as the reference's 2-rank
                             allreduce_packet plan.
  allreduce_rres_n{N}.json   Simple protocol: relaxed handshake, rres (read the peers' chunk,
                             reduce, write the result into every rank's input), then a
                             signal/wait so no rank leaves early.  Same operation mix as the
                             reference's allreduce plan.
  allreduce_put_n{N}.json    Simple protocol through scratch: put my copy of chunk q into rank q's
                             scratch, signal/wait, re (my chunk + the scratch copies), put the
                             result into every peer's output, then a workgroup barrier and a
                             semaphore hand-off between the threadblocks; exercises put, re, copy,
                             barrier, sem_acquire/sem_release and pipeline.

and of the plans that bring the remaining device operations onto a GPU (each generator's docstring
says how its reads and writes are ordered):

  allgather_get_n{N}.json      AllGather by `get` from the peers' outputs.
  get_offsets_n2.json          Not a collective: `get` with differing source and destination chunks.
  reducescatter_rre_n{N}.json  ReduceScatter by `rre` from the peers' inputs.
  allreduce_res_n{N}.json      pws / pwsf into the owners' scratch, `res` to every output, flush.
  allreduce_relay_n{N}.json    LL: recspkt / rppkt ring relay, and repkt + cpkt and recpkt groups.
  allreduce_reuse_n{N}.json    reuse_resources with 4096 scratch chunks: a pipeline through wrapped
                               16384-byte scratch windows (`re` + put at 2 ranks, `res` at 4).

`_min` in a name is the same generator with reduce_op min, `_a4` / `_a8` with that buffer_alignment.

Run:  python tests/golden/plans/make_plans.py   (rewrites the .json files next to it)
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _common(name, protocol, gpus, nthreads=1024, double=False, inplace=True, collective="allreduce", reuse=False,
            align=16):
    return {"name": name, "collective": collective, "protocol": protocol, "inplace": inplace,
            "reuse_resources": reuse, "gpus": gpus, "num_threads_per_block": nthreads,
            "use_double_scratch_buffer": double, "buffer_alignment": align, "min_message_size": 0,
            "max_message_size": 2**64 - 1}


def _tbg(op, t, T):
    if T > 1:
        op["tbg_info"] = {"tb_id": t, "tbg_size": T}
    return op


def _tag(op="sum", align=16):
    """Name suffix of a variant: reduce operation and buffer alignment."""
    return ("_min" if op == "min" else "") + (f"_a{align}" if align != 16 else "")


def allreduce_pkt(n, T=2, nthreads=512, align=16):
    gpus = []
    for r in range(n):
        peers = [q for q in range(n) if q != r]
        # remote buffer k = peer peers[k]'s scratch; channel k = peer peers[k]
        tbs = []
        for t in range(T):
            ops = []
            ops.append(_tbg({"name": "ppkt", "src_buff": [{"type": "i", "index": q, "size": 1} for q in peers],
                             "dst_buff": [{"buffer_id": k, "index": r, "size": 1} for k, _ in enumerate(peers)],
                             "channel_type": "memory"}, t, T))
            ops.append(_tbg({"name": "respkt",
                             "src_buff": [{"type": "i", "index": r, "size": 1}] +
                                         [{"type": "s", "index": q, "size": 1} for q in peers],
                             "dst_buff": [{"type": "i", "index": r, "size": 1}] +
                                         [{"buffer_id": k, "index": n + r, "size": 1} for k, _ in enumerate(peers)],
                             "channel_type": "memory", "reduce_op": "sum"}, t, T))
            for q in peers:
                ops.append(_tbg({"name": "upkt", "src_buff": [{"type": "s", "index": n + q, "size": 1}],
                                 "dst_buff": [{"type": "i", "index": q, "size": 1}]}, t, T))
            tbs.append({"id": t, "ops": ops,
                        "channels": [{"channel_type": "memory", "channel_ids": list(range(len(peers)))}],
                        "remote_buffer_refs": [{"access_channel_type": "memory",
                                                "remote_buffer_ids": list(range(len(peers)))}]})
        gpus.append({"id": r, "input_chunks": n, "output_chunks": n, "scratch_chunks": 2 * n, "threadblocks": tbs,
                     "channels": [{"channel_type": "memory", "connected_to": peers}],
                     "remote_buffers": [{"rank": q, "type": "s", "access_channel_types": ["memory"]} for q in peers],
                     "semaphores": []})
    return _common(f"allreduce_pkt{_tag(align=align)}_n{n}", "LL", gpus, nthreads=nthreads, double=True, align=align)


def allreduce_rres(n, per_rank_tbs=2, nthreads=512, op="sum"):
    """Chunks: n * per_rank_tbs; rank r owns chunks [r*P, (r+1)*P), one threadblock per chunk."""
    P = per_rank_tbs
    gpus = []
    for r in range(n):
        peers = [q for q in range(n) if q != r]
        # channels: for every threadblock one channel to every peer (channel id = t*(n-1)+k)
        conn = []
        for _t in range(P):
            conn.extend(peers)
        tbs = []
        for t in range(P):
            chunk = r * P + t
            chans = [t * (n - 1) + k for k in range(n - 1)]
            local_ids = list(range(n - 1))
            ops = [
                {"name": "rlxsignal", "channel_ids": local_ids, "channel_type": "memory"},
                {"name": "rlxwait", "channel_ids": local_ids, "channel_type": "memory"},
                {"name": "nop"},
                {"name": "rres",
                 "src_buff": [{"type": "i", "index": chunk, "size": 1}] +
                             [{"buffer_id": k, "index": chunk, "size": 1} for k in range(n - 1)],
                 "dst_buff": [{"type": "i", "index": chunk, "size": 1}] +
                             [{"buffer_id": k, "index": chunk, "size": 1} for k in range(n - 1)],
                 "channel_type": "memory", "reduce_op": op},
                {"name": "nop"},
                {"name": "signal", "channel_ids": local_ids, "channel_type": "memory"},
                {"name": "wait", "channel_ids": local_ids, "channel_type": "memory"},
            ]
            tbs.append({"id": t, "ops": ops, "channels": [{"channel_type": "memory", "channel_ids": chans}],
                        "remote_buffer_refs": [{"access_channel_type": "memory", "remote_buffer_ids": list(range(n - 1))}]})
        gpus.append({"id": r, "input_chunks": n * P, "output_chunks": n * P, "scratch_chunks": 0, "threadblocks": tbs,
                     "channels": [{"channel_type": "memory", "connected_to": conn}],
                     "remote_buffers": [{"rank": q, "type": "i", "access_channel_types": ["memory"]} for q in peers],
                     "semaphores": []})
    return _common(f"allreduce_rres{_tag(op)}_n{n}", "Simple", gpus, nthreads=nthreads)


def allreduce_put(n, nthreads=256, unit=4096, op="sum", align=16):
    """Out-of-place.  tb0: puts + reduction; tb1: waits on tb0 through a semaphore, then copies the
    reduced own chunk into the output in a pipeline of `unit`-byte steps.  Remote buffers: peers'
    scratch (put targets) and peers' outputs (result targets)."""
    gpus = []
    for r in range(n):
        peers = [q for q in range(n) if q != r]
        scr = list(range(n - 1))              # remote buffer ids: scratch of peers[k]
        outs = list(range(n - 1, 2 * (n - 1)))  # remote buffer ids: output of peers[k]
        tb0 = [
            {"name": "put", "src_buff": [{"type": "i", "index": q, "size": 1} for q in peers],
             "dst_buff": [{"buffer_id": k, "index": r, "size": 1} for k in range(n - 1)], "channel_type": "memory"},
            {"name": "nop"},
            {"name": "signal", "channel_ids": list(range(n - 1)), "channel_type": "memory"},
            {"name": "wait", "channel_ids": list(range(n - 1)), "channel_type": "memory"},
            {"name": "nop"},
            {"name": "re", "src_buff": [{"type": "i", "index": r, "size": 1}] +
                                       [{"type": "s", "index": q, "size": 1} for q in peers],
             "dst_buff": [{"type": "s", "index": r, "size": 1}], "reduce_op": op},
            {"name": "put", "src_buff": [{"type": "s", "index": r, "size": 1} for _ in peers],
             "dst_buff": [{"buffer_id": n - 1 + k, "index": r, "size": 1} for k in range(n - 1)],
             "channel_type": "memory"},
            {"name": "sem_release", "semaphore_ids": [0]},
            {"name": "barrier", "barrier_id": 0, "num_threadblocks": 2},
            {"name": "signal", "channel_ids": list(range(n - 1)), "channel_type": "memory"},
            {"name": "wait", "channel_ids": list(range(n - 1)), "channel_type": "memory"},
        ]
        tb1 = [
            {"name": "sem_acquire", "semaphore_ids": [0]},
            {"name": "pipeline", "iter_context": {"unit_size": unit, "num_chunks": 1},
             "ops": [{"name": "copy", "src_buff": [{"type": "s", "index": r, "size": 1}],
                      "dst_buff": [{"type": "o", "index": r, "size": 1}]}]},
            {"name": "barrier", "barrier_id": 0, "num_threadblocks": 2},
        ]
        gpus.append({"id": r, "input_chunks": n, "output_chunks": n, "scratch_chunks": n,
                     "threadblocks": [
                         {"id": 0, "ops": tb0, "channels": [{"channel_type": "memory", "channel_ids": list(range(n - 1))}],
                          "remote_buffer_refs": [{"access_channel_type": "memory", "remote_buffer_ids": scr + outs}]},
                         {"id": 1, "ops": tb1}],
                     "channels": [{"channel_type": "memory", "connected_to": peers}],
                     "remote_buffers": [{"rank": q, "type": "s", "access_channel_types": ["memory"]} for q in peers] +
                                       [{"rank": q, "type": "o", "access_channel_types": ["memory"]} for q in peers],
                     "semaphores": [{"init_value": 0}]})
    return _common(f"allreduce_put{_tag(op, align)}_n{n}", "Simple", gpus, nthreads=nthreads, inplace=False, align=align)


def _mesh_tb(t, n, ops, nremote=None):
    """Threadblock t with its own channel to every peer (channel id t*(n-1)+k, so tag t between each
    pair of ranks) and the first `nremote` remote buffers."""
    nremote = n - 1 if nremote is None else nremote
    return {"id": t, "ops": ops,
            "channels": [{"channel_type": "memory", "channel_ids": [t * (n - 1) + k for k in range(n - 1)]}],
            "remote_buffer_refs": [{"access_channel_type": "memory", "remote_buffer_ids": list(range(nremote))}]}


def _sync(n, relaxed=False):
    ids = list(range(n - 1))
    pre = "rlx" if relaxed else ""
    return [{"name": pre + "signal", "channel_ids": ids, "channel_type": "memory"},
            {"name": pre + "wait", "channel_ids": ids, "channel_type": "memory"}]


def _remote(peers, types):
    return [{"rank": q, "type": ty, "access_channel_types": ["memory"]} for ty in types for q in peers]


def allgather_get(n, T=2, nthreads=256):
    """Out of place, input_chunks 1, output_chunks n.  Threadblock t handles slice t of every chunk:
    copy my input into output chunk r, signal / wait every peer's threadblock t (its copy is done),
    get chunk q from peer q's output into my output chunk q, and a closing signal / wait: nobody
    overwrites its output chunk in the next call while a peer still reads it."""
    gpus = []
    for r in range(n):
        peers = [q for q in range(n) if q != r]
        tbs = []
        for t in range(T):
            ops = [_tbg({"name": "copy", "src_buff": [{"type": "i", "index": 0, "size": 1}],
                         "dst_buff": [{"type": "o", "index": r, "size": 1}]}, t, T),
                   {"name": "nop"}] + _sync(n) + [
                   _tbg({"name": "get", "src_buff": [{"buffer_id": k, "index": q, "size": 1} for k, q in enumerate(peers)],
                         "dst_buff": [{"type": "o", "index": q, "size": 1} for q in peers],
                         "channel_type": "memory"}, t, T),
                   {"name": "nop"}] + _sync(n)
            tbs.append(_mesh_tb(t, n, ops))
        gpus.append({"id": r, "input_chunks": 1, "output_chunks": n, "scratch_chunks": 0, "threadblocks": tbs,
                     "channels": [{"channel_type": "memory", "connected_to": peers * T}],
                     "remote_buffers": _remote(peers, "o"), "semaphores": []})
    return _common(f"allgather_get_n{n}", "Simple", gpus, nthreads=nthreads, inplace=False, collective="allgather")


def get_offsets(nthreads=256):
    """Two ranks, not a collective: pins how `get` addresses its two sides.  The reference's handler
    (execution_kernel.hpp:129-142) adds the SOURCE offset to the local pointer and the DESTINATION
    offset to the remote one, so `get src=[peer input, index 1] dst=[output, index 0]` reads the
    peer's input chunk 0 into my output chunk 1.  A local copy of my input chunk 1 fills output
    chunk 0, so the whole output is defined: [my input chunk 1, the peer's input chunk 0]."""
    gpus = []
    for r in range(2):
        peers = [1 - r]
        ops = _sync(2, relaxed=True) + [
            {"name": "nop"},  # a relaxed wait holds only its polling lanes: the workgroup meets here
            {"name": "copy", "src_buff": [{"type": "i", "index": 1, "size": 1}],
             "dst_buff": [{"type": "o", "index": 0, "size": 1}]},
            {"name": "get", "src_buff": [{"buffer_id": 0, "index": 1, "size": 1}],
             "dst_buff": [{"type": "o", "index": 0, "size": 1}], "channel_type": "memory"},
            {"name": "nop"}] + _sync(2)
        gpus.append({"id": r, "input_chunks": 2, "output_chunks": 2, "scratch_chunks": 0,
                     "threadblocks": [_mesh_tb(0, 2, ops)],
                     "channels": [{"channel_type": "memory", "connected_to": peers}],
                     "remote_buffers": _remote(peers, "i"), "semaphores": []})
    return _common("get_offsets_n2", "Simple", gpus, nthreads=nthreads, inplace=False, collective="get_offsets")


def reducescatter_rre(n, T=2, nthreads=256, op="sum", align=16):
    """Out of place, input_chunks n, output_chunks 1.  Relaxed handshake (every peer's kernel of this
    call runs, so its input is this call's), rre of slice t of my chunk from every peer's input
    into my output, then signal / wait: no rank's input changes while a peer still reads it."""
    gpus = []
    for r in range(n):
        peers = [q for q in range(n) if q != r]
        tbs = []
        for t in range(T):
            ops = _sync(n, relaxed=True) + [
                {"name": "nop"},
                _tbg({"name": "rre", "src_buff": [{"type": "i", "index": r, "size": 1}] +
                                                 [{"buffer_id": k, "index": r, "size": 1} for k in range(n - 1)],
                      "dst_buff": [{"type": "o", "index": 0, "size": 1}], "channel_type": "memory",
                      "reduce_op": op}, t, T),
                {"name": "nop"}] + _sync(n)
            tbs.append(_mesh_tb(t, n, ops))
        gpus.append({"id": r, "input_chunks": n, "output_chunks": 1, "scratch_chunks": 0, "threadblocks": tbs,
                     "channels": [{"channel_type": "memory", "connected_to": peers * T}],
                     "remote_buffers": _remote(peers, "i"), "semaphores": []})
    return _common(f"reducescatter_rre{_tag(op, align)}_n{n}", "Simple", gpus, nthreads=nthreads, inplace=False,
                   collective="reducescatter", align=align)


def allreduce_res(n, T=2, nthreads=256):
    """Out of place through scratch.  Threadblock t, slice t of every chunk: pws (t even) or pwsf
    (t odd) my copy of chunk q into rank q's scratch slot r, signal / wait, res (my chunk + the
    scratch copies in peer order) into my output and every peer's output, flush, signal / wait.  The
    closing signal / wait orders the next call's puts after this call's reads of the same slots and
    keeps a rank from leaving before the peers' results have landed in its output."""
    gpus = []
    for r in range(n):
        peers = [q for q in range(n) if q != r]
        tbs = []
        for t in range(T):
            ops = [_tbg({"name": "pws" if t % 2 == 0 else "pwsf",
                         "src_buff": [{"type": "i", "index": q, "size": 1} for q in peers],
                         "dst_buff": [{"buffer_id": k, "index": r, "size": 1} for k in range(n - 1)],
                         "channel_type": "memory"}, t, T),
                   {"name": "nop"}] + _sync(n) + [
                   _tbg({"name": "res", "src_buff": [{"type": "i", "index": r, "size": 1}] +
                                                    [{"type": "s", "index": q, "size": 1} for q in peers],
                         "dst_buff": [{"type": "o", "index": r, "size": 1}] +
                                     [{"buffer_id": n - 1 + k, "index": r, "size": 1} for k in range(n - 1)],
                         "channel_type": "memory", "reduce_op": "sum"}, t, T),
                   {"name": "flush", "channel_ids": list(range(n - 1)), "channel_type": "memory"},
                   {"name": "nop"}] + _sync(n)
            tbs.append(_mesh_tb(t, n, ops, nremote=2 * (n - 1)))
        gpus.append({"id": r, "input_chunks": n, "output_chunks": n, "scratch_chunks": n, "threadblocks": tbs,
                     "channels": [{"channel_type": "memory", "connected_to": peers * T}],
                     "remote_buffers": _remote(peers, "so"), "semaphores": []})
    return _common(f"allreduce_res_n{n}", "Simple", gpus, nthreads=nthreads, inplace=False)


def allreduce_relay(n, nthreads=256, op="sum"):
    """LL protocol, out of place, three threadblocks that each take a third of every chunk
    (tbg_info) with a different operation mix.  Packet slots (in payload-chunk units of the scratch):
    q < n holds rank q's contribution to my chunk, n + c holds the reduced chunk c.

      tb0  ppkt to the owners; recspkt: reduced chunk r -> my output, my slot n+r and the next
           rank's slot n+r; rppkt relays: my slot n+r to the previous rank (n > 2), and the chunks
           that arrived from the previous rank on to the next one until every rank has them; upkt.
      tb1  ppkt; repkt -> my output chunk r; nop; cpkt of that output chunk into my slot n+r;
           rppkt of that slot to every peer; upkt of the peers' chunks.
      tb2  ppkt; recpkt -> my output chunk r and my slot n+r; rppkt of that slot to every peer; upkt.

    No channels: packets carry the call's flag and the scratch is double buffered, so a call can
    only overwrite a slot of the call before last, which every rank has left (it sent this
    threadblock the packets of the call in between)."""
    gpus = []
    for r in range(n):
        peers = [q for q in range(n) if q != r]
        rb = {q: k for k, q in enumerate(peers)}  # remote buffer id of peer q's scratch
        nxt, prv = (r + 1) % n, (r - 1) % n
        own = [{"type": "i", "index": r, "size": 1}] + [{"type": "s", "index": q, "size": 1} for q in peers]

        def ppkt(t):
            return _tbg({"name": "ppkt", "src_buff": [{"type": "i", "index": q, "size": 1} for q in peers],
                         "dst_buff": [{"buffer_id": rb[q], "index": r, "size": 1} for q in peers],
                         "channel_type": "memory"}, t, 3)

        def rppkt(t, c, dsts):
            return _tbg({"name": "rppkt", "src_buff": [{"type": "s", "index": n + c, "size": 1}],
                         "dst_buff": [{"buffer_id": rb[q], "index": n + c, "size": 1} for q in dsts],
                         "channel_type": "memory"}, t, 3)

        def upkts(t):
            return [_tbg({"name": "upkt", "src_buff": [{"type": "s", "index": n + q, "size": 1}],
                          "dst_buff": [{"type": "o", "index": q, "size": 1}]}, t, 3) for q in peers]

        tb0 = [ppkt(0),
               _tbg({"name": "recspkt", "src_buff": own,
                     "dst_buff": [{"type": "o", "index": r, "size": 1}, {"type": "s", "index": n + r, "size": 1},
                                  {"buffer_id": rb[nxt], "index": n + r, "size": 1}],
                     "channel_type": "memory", "reduce_op": op}, 0, 3)]
        if n > 2:
            tb0.append(rppkt(0, r, [prv]))
        tb0 += [rppkt(0, (r - j) % n, [nxt]) for j in range(1, n - 2)]
        tb0 += upkts(0)
        tb1 = [ppkt(1),
               _tbg({"name": "repkt", "src_buff": own, "dst_buff": [{"type": "o", "index": r, "size": 1}],
                     "reduce_op": op}, 1, 3),
               {"name": "nop"},
               _tbg({"name": "cpkt", "src_buff": [{"type": "o", "index": r, "size": 1}],
                     "dst_buff": [{"type": "s", "index": n + r, "size": 1}]}, 1, 3),
               rppkt(1, r, peers)] + upkts(1)
        tb2 = [ppkt(2),
               _tbg({"name": "recpkt", "src_buff": own,
                     "dst_buff": [{"type": "o", "index": r, "size": 1}, {"type": "s", "index": n + r, "size": 1}],
                     "reduce_op": op}, 2, 3),
               rppkt(2, r, peers)] + upkts(2)
        refs = [{"access_channel_type": "memory", "remote_buffer_ids": list(range(n - 1))}]
        gpus.append({"id": r, "input_chunks": n, "output_chunks": n, "scratch_chunks": 2 * n,
                     "threadblocks": [{"id": t, "ops": ops, "channels": [], "remote_buffer_refs": refs}
                                      for t, ops in enumerate((tb0, tb1, tb2))],
                     "channels": [], "remote_buffers": _remote(peers, "s"), "semaphores": []})
    return _common(f"allreduce_relay{_tag(op)}_n{n}", "LL", gpus, nthreads=nthreads, double=True, inplace=False)


def allreduce_reuse(n, send=False, op="sum", unit=4096, nthreads=256):
    """reuse_resources with scratch_chunks 4096: a scratch chunk is a 16384-byte window, and once a
    message chunk is larger the pipeline's offsets wrap inside it.  One threadblock, one pipeline
    over my chunk in `unit`-byte steps; every step: put my piece of chunk q into rank q's window r,
    signal / wait, reduce my piece + the windows -- `re` into my output followed by a put of the
    result into every peer's output, or (`send`) one `res` doing both -- and a signal / wait back.
    The steps are in lockstep across ranks, so a window slot is rewritten (four steps later) only
    after its reader has signalled that step's end."""
    gpus = []
    for r in range(n):
        peers = [q for q in range(n) if q != r]
        src = [{"type": "i", "index": r, "size": 1}] + [{"type": "s", "index": q, "size": 1} for q in peers]
        remote_out = [{"buffer_id": n - 1 + k, "index": r, "size": 1} for k in range(n - 1)]
        inner = [{"name": "put", "src_buff": [{"type": "i", "index": q, "size": 1} for q in peers],
                  "dst_buff": [{"buffer_id": k, "index": r, "size": 1} for k in range(n - 1)], "channel_type": "memory"},
                 {"name": "nop"}] + _sync(n)
        if send:
            inner += [{"name": "res", "src_buff": src, "dst_buff": [{"type": "o", "index": r, "size": 1}] + remote_out,
                       "channel_type": "memory", "reduce_op": op}]
        else:
            inner += [{"name": "re", "src_buff": src, "dst_buff": [{"type": "o", "index": r, "size": 1}], "reduce_op": op},
                      {"name": "nop"},
                      {"name": "put", "src_buff": [{"type": "o", "index": r, "size": 1} for _ in peers],
                       "dst_buff": remote_out, "channel_type": "memory"}]
        inner += [{"name": "nop"}] + _sync(n)
        ops = [{"name": "pipeline", "iter_context": {"unit_size": unit, "num_chunks": 1}, "ops": inner}]
        gpus.append({"id": r, "input_chunks": n, "output_chunks": n, "scratch_chunks": 4096,
                     "threadblocks": [_mesh_tb(0, n, ops, nremote=2 * (n - 1))],
                     "channels": [{"channel_type": "memory", "connected_to": peers}],
                     "remote_buffers": _remote(peers, "so"), "semaphores": []})
    return _common(f"allreduce_reuse{_tag(op)}_n{n}", "Simple", gpus, nthreads=nthreads, inplace=False, reuse=True)


PLANS = {
    "allreduce_pkt_n2.json": lambda: allreduce_pkt(2, T=2),
    "allreduce_pkt_n4.json": lambda: allreduce_pkt(4, T=2),
    "allreduce_pkt_n8.json": lambda: allreduce_pkt(8, T=4),
    "allreduce_rres_n2.json": lambda: allreduce_rres(2, per_rank_tbs=4),
    "allreduce_rres_n4.json": lambda: allreduce_rres(4, per_rank_tbs=2),
    "allreduce_put_n2.json": lambda: allreduce_put(2),
    "allreduce_put_n4.json": lambda: allreduce_put(4),
    # every other executeOp case: get, rre, res / pws / pwsf / flush, the packet relays
    "allgather_get_n2.json": lambda: allgather_get(2),
    "allgather_get_n4.json": lambda: allgather_get(4),
    "allgather_get_n8.json": lambda: allgather_get(8, T=1),
    "get_offsets_n2.json": get_offsets,
    "reducescatter_rre_n2.json": lambda: reducescatter_rre(2),
    "reducescatter_rre_n4.json": lambda: reducescatter_rre(4),
    "allreduce_res_n2.json": lambda: allreduce_res(2),
    "allreduce_res_n4.json": lambda: allreduce_res(4),
    "allreduce_relay_n2.json": lambda: allreduce_relay(2),
    "allreduce_relay_n4.json": lambda: allreduce_relay(4),
    # reuse_resources: re + put at two ranks, res at four
    "allreduce_reuse_n2.json": lambda: allreduce_reuse(2),
    "allreduce_reuse_n4.json": lambda: allreduce_reuse(4, send=True),
    # reduce_op min
    "allreduce_rres_min_n2.json": lambda: allreduce_rres(2, per_rank_tbs=4, op="min"),
    "allreduce_rres_min_n4.json": lambda: allreduce_rres(4, per_rank_tbs=2, op="min"),
    "reducescatter_rre_min_n2.json": lambda: reducescatter_rre(2, op="min"),
    "reducescatter_rre_min_n4.json": lambda: reducescatter_rre(4, op="min"),
    "allreduce_put_min_n2.json": lambda: allreduce_put(2, op="min"),
    "allreduce_reuse_min_n2.json": lambda: allreduce_reuse(2, op="min"),
    "allreduce_relay_min_n2.json": lambda: allreduce_relay(2, op="min"),
    # buffer_alignment below 16: 4 for Simple and LL8, 8 for LL16
    "allreduce_put_a4_n2.json": lambda: allreduce_put(2, align=4),
    "reducescatter_rre_a4_n2.json": lambda: reducescatter_rre(2, align=4),
    "allreduce_put_min_a4_n2.json": lambda: allreduce_put(2, op="min", align=4),   # min in the 4-byte tails
    "reducescatter_rre_min_a4_n2.json": lambda: reducescatter_rre(2, op="min", align=4),
    "allreduce_pkt_a4_n2.json": lambda: allreduce_pkt(2, T=2, align=4),
    "allreduce_pkt_a8_n2.json": lambda: allreduce_pkt(2, T=2, align=8),
}


def main():
    for fname, fn in PLANS.items():
        with open(os.path.join(HERE, fname), "w") as f:
            json.dump(fn(), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
