"""Export + serving: the counterpart of the reference's BestExporter block (/root/reference
algorithm/DeepFM/deepfm.py:307-321; the same block in every model script):

    feature_spec = tf.feature_column.make_parse_example_spec(total_feature_columns)
    serving_input_receiver_fn = tf.estimator.export.build_parsing_serving_input_receiver_fn(feature_spec)
    exporters = [tf.estimator.BestExporter(name="best_exporter", serving_input_receiver_fn=..., exports_to_keep=5)]
    eval_spec = tf.estimator.EvalSpec(..., exporters=exporters)

TF writes a SavedModel (graph + variables) whose serving signature takes a batch of serialized tf.train.Example
protos.  Here a model is its model_fn + params (code) and its variables: an export is a directory

    <model_dir>/export/<exporter name>/<unix seconds>/variables.npz      {reference TF variable name: array}
                                                       serving.json       receiver feature spec, prediction keys, eval result

and `ServingModel(model_fn, params, export_dir)` is the serving side: `predict(serialized_examples)` parses the protos
with the exported feature spec (the parsing receiver) and runs the PREDICT graph on the HIP kernels; `serve` is the same
contract with the native decoder of include/recalgo_host.h in front and, after `compile(batch_sizes)`, one captured graph per
batch bucket behind it (DESIGN.md §5 "Serving").  The variable file
uses the reference's names and shapes (Estimator.export_variables), so it is interchangeable with a dump of a
reference-trained TF checkpoint (scripts/tf_ckpt_to_npz.py) — either loads into either.
"""
from __future__ import annotations

import json
import os
import shutil
import time
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np



def build_parsing_serving_input_receiver_fn(feature_spec: dict) -> Callable[[Sequence[bytes]], dict]:
    """tf.estimator.export.build_parsing_serving_input_receiver_fn: the returned receiver turns a batch of serialized
    tf.train.Example protos into the features dict the model_fn takes (tf.parse_example semantics)."""
    def receiver(serialized_examples: Sequence[bytes]) -> dict:
        from .algorithm.utils import parse_example
        return parse_example(list(serialized_examples), feature_spec)
    receiver.feature_spec = feature_spec
    return receiver


def _spec_to_json(feature_spec: dict) -> dict:
    out = {}
    for key, s in feature_spec.items():
        kind = s[0]
        if kind == "fixed":
            _, dtype, shape, default = s
            out[key] = {"kind": "fixed", "dtype": np.dtype(dtype).name, "shape": list(shape),
                        "default": None if default is None else float(default)}
        else:
            out[key] = {"kind": kind, "dtype": "string" if len(s) < 2 or s[1] in (bytes, str, np.bytes_, None) else np.dtype(s[1]).name}
    return out


def _spec_from_json(js: dict) -> dict:
    out = {}
    for key, s in js.items():
        if s["kind"] == "fixed":
            out[key] = ("fixed", np.dtype(s["dtype"]).type, tuple(s["shape"]), s["default"])
        else:
            out[key] = (s["kind"], np.bytes_ if s["dtype"] == "string" else np.dtype(s["dtype"]).type)
    return out


def export_model(estimator, export_dir_base: str, serving_input_receiver_fn, eval_result: Optional[dict] = None) -> str:
    """Estimator.export_saved_model: one timestamped directory under export_dir_base; returns its path."""
    os.makedirs(export_dir_base, exist_ok=True)
    stamp = int(time.time())
    while os.path.exists(os.path.join(export_dir_base, str(stamp))):       # TF also bumps a colliding timestamp
        stamp += 1
    final = os.path.join(export_dir_base, str(stamp))
    tmp = os.path.join(export_dir_base, f"temp-{stamp}")
    os.makedirs(tmp)
    np.savez(os.path.join(tmp, "variables.npz"), **estimator.export_variables())
    meta = {"feature_spec": _spec_to_json(getattr(serving_input_receiver_fn, "feature_spec", {})),
            "global_step": int(getattr(estimator, "global_step", 0)),
            "eval_result": {k: float(v) for k, v in (eval_result or {}).items()},
            "signature": "serialized tf.train.Example protos -> model_fn(mode=PREDICT).predictions"}
    with open(os.path.join(tmp, "serving.json"), "w") as f:
        json.dump(meta, f, indent=1)
    os.replace(tmp, final)                                                  # readers never see a half-written export
    return final


def _loss_smaller(best_eval_result: dict, current_eval_result: dict) -> bool:
    """tf.estimator.BestExporter's default compare_fn: a strictly smaller `loss` is better."""
    for r in (best_eval_result, current_eval_result):
        if not r or "loss" not in r:
            raise ValueError("BestExporter: the evaluation result has no 'loss'")
    return float(current_eval_result["loss"]) < float(best_eval_result["loss"])


class BestExporter:
    """tf.estimator.BestExporter: exports after an evaluation only when it is the best so far, keeps the newest
    `exports_to_keep` exports.  The best result is remembered across runs (TF re-reads it from the eval event files;
    here from the newest export's serving.json)."""

    def __init__(self, name: str = "best_exporter", serving_input_receiver_fn=None, exports_to_keep: Optional[int] = 5,
                 compare_fn: Callable[[dict, dict], bool] = _loss_smaller, **_ignored):
        if serving_input_receiver_fn is None:
            raise ValueError("BestExporter: serving_input_receiver_fn is required")
        if exports_to_keep is not None and exports_to_keep <= 0:
            raise ValueError("BestExporter: exports_to_keep must be positive or None")
        self.name, self.receiver, self.exports_to_keep, self.compare_fn = name, serving_input_receiver_fn, exports_to_keep, compare_fn
        self._best: Optional[dict] = None

    def _recover_best(self, export_path: str) -> None:
        if self._best is not None or not os.path.isdir(export_path):
            return
        for d in sorted(list_exports(export_path), key=_stamp, reverse=True):
            try:
                with open(os.path.join(d, "serving.json")) as f:
                    r = json.load(f).get("eval_result")
                if r and "loss" in r:
                    self._best = r
                    return
            except (OSError, ValueError):
                continue

    def export(self, estimator, export_path: str, checkpoint_path: Optional[str], eval_result: dict,
               is_the_final_export: bool = False) -> Optional[str]:
        self._recover_best(export_path)
        if self._best is not None and not self.compare_fn(self._best, eval_result):
            return None
        self._best = dict(eval_result)
        out = export_model(estimator, export_path, self.receiver, eval_result)
        if self.exports_to_keep is not None:
            for old in sorted(list_exports(export_path), key=_stamp)[:-self.exports_to_keep]:
                shutil.rmtree(old, ignore_errors=True)
        return out


def list_exports(export_path: str) -> List[str]:
    """The timestamped export directories under export_path (temp-* leftovers are not exports)."""
    if not os.path.isdir(export_path):
        return []
    return [os.path.join(export_path, d) for d in os.listdir(export_path)
            if d.isdigit() and os.path.isfile(os.path.join(export_path, d, "variables.npz"))]


def _stamp(path: str) -> int:
    return int(os.path.basename(path))


def latest_export(export_path: str) -> Optional[str]:
    ex = sorted(list_exports(export_path), key=_stamp)
    return ex[-1] if ex else None


def plan_chunks(n: int, buckets: Sequence[int]) -> List[tuple]:
    """How a request of n rows runs on graphs captured for the batch sizes `buckets`: [(first row, rows, bucket)], in row
    order, every row once.  Full chunks of the largest bucket while more than that is left, then the smallest bucket that
    holds the rest (padded up to it).  Pure: no device, no model."""
    sizes = sorted({int(b) for b in buckets})
    if not sizes or sizes[0] < 1:
        raise ValueError(f"plan_chunks: the buckets must be positive batch sizes, got {list(buckets)}")
    n = int(n)
    if n < 0:
        raise ValueError("plan_chunks: a request has no negative number of rows")
    out, at = [], 0
    while n - at > sizes[-1]:
        out.append((at, sizes[-1], sizes[-1]))
        at += sizes[-1]
    if n - at > 0:
        out.append((at, n - at, next(b for b in sizes if b >= n - at)))
    return out


def fold_batch_norms(arrays: Dict[str, "torch.Tensor"], epsilon: Optional[float] = None) -> dict:
    """{<scope>/gamma: (scale, shift)} of every BatchNorm among the named arrays of a model (<scope>/gamma, beta, moving_mean,
    moving_variance): nn.fold_batch_norm on each, computed once when an export is compiled.  Pure."""
    from . import nn
    eps = nn.BN_EPSILON if epsilon is None else float(epsilon)
    out = {}
    for name in arrays:
        if name.endswith("/gamma"):
            scope = name[:-len("gamma")]
            parts = [arrays.get(scope + k) for k in ("beta", "moving_mean", "moving_variance")]
            if all(p is not None for p in parts):
                out[name] = tuple(t.contiguous() for t in nn.fold_batch_norm(arrays[name], *parts, eps))
    return out


def _columns_by_key(params: dict) -> dict:
    """feature key -> the CategoricalColumn / NumericColumn behind it, from every column (list) among a model's params"""
    from .feature_column import CategoricalColumn, NumericColumn
    found: dict = {}

    def visit(o):
        if isinstance(o, (list, tuple)):
            for v in o:
                visit(v)
            return
        base = getattr(o, "categorical_column", o)
        for c in getattr(base, "keys", None) or [base]:                  # (a crossed column: its two key columns)
            if isinstance(c, (CategoricalColumn, NumericColumn)):
                found.setdefault(c.key, c)
    for v in params.values():
        visit(v)
    return found


def ragged_span_layout(rows: int, F: int, NF: int, caps):
    """The staging / static-input layout of a bucket of `rows` rows whose model has bags or histories: the dense layout of
    ServingModel._span_bytes(rows, F, NF), then for every (key, values per row) of `caps`, in that order,
        offsets int64 [rows + 1] | values int64 [rows * cap]
    each piece starting on a 16-byte boundary.  -> ({key: (byte offset of offsets, byte offset of values, rows * cap)}, bytes)"""
    up = lambda n: (int(n) + 15) // 16 * 16
    at = up(ServingModel._span_bytes(rows, F, NF)[1])
    pieces = {}
    for key, cap in caps:
        off_at = at
        val_at = off_at + up((rows + 1) * 8)
        at = val_at + up(max(rows * int(cap), 1) * 8)
        pieces[key] = (off_at, val_at, rows * int(cap))
    return pieces, at


def _fill_ragged_pieces(host, pieces, bags, rows: int, n: int) -> bool:
    """Writes the decoded bags of an n-row request into the pieces of a `rows`-row span (numpy uint8 `host`): offsets, the rows
    past the request as empty bags; values, then -1 up to the capacity.  A bag that does not fit is NOT truncated: every piece
    is written as empty bags and False is returned."""
    fits = all(int(bags[key][0][n]) <= cap for key, (_, _, cap) in pieces.items())
    for key, (off_at, val_at, cap) in pieces.items():
        offsets, values = bags[key]
        o = host[off_at:off_at + (rows + 1) * 8].view(np.int64)
        v = host[val_at:val_at + cap * 8].view(np.int64)
        nnz = int(offsets[n]) if fits else 0
        o[:n + 1] = offsets[:n + 1] if fits else 0
        o[n + 1:] = nnz
        v[:nnz] = values[:nnz]
        v[nnz:] = -1
    return fits


class _Bucket:
    """One captured PREDICT graph: its static input span (ids, then floats, then the ragged pieces: the staging layout), the
    feature views over it, the static outputs, and the serving plan whose BatchNorm folds the captured tower reads."""
    __slots__ = ("rows", "span", "features", "graph", "out", "tower", "plan", "caps")


class ServingModel:
    """The serving side of an export: model_fn + params (the code) + an export directory (the variables and the
    receiver's feature spec).

        predict(serialized tf.train.Example protos) -> {prediction key: array [n, ...]}     Python decode, eager model_fn
        serve(protos)                                -> the same dict                        native decode (recalgo_examples_*),
                                                                                             then the compiled graph of the
                                                                                             request's bucket — or, without
                                                                                             compile(), the eager model_fn
        compile(batch_sizes)                         captures the PREDICT graph once per bucket size"""

    DECODE_THREADS = 4            # recalgo_examples_decode's `threads` for requests of 256 rows and more (never the host's core count)

    def __init__(self, model_fn, params: dict, export_dir: str, device=None):
        from .estimator import Estimator, RunConfig
        with open(os.path.join(export_dir, "serving.json")) as f:
            self.meta = json.load(f)
        self.feature_spec = _spec_from_json(self.meta["feature_spec"])
        self.receiver = build_parsing_serving_input_receiver_fn(self.feature_spec)
        self.estimator = Estimator(model_fn, params, RunConfig(device=device))
        self._variables = dict(np.load(os.path.join(export_dir, "variables.npz")))
        self._loaded = False
        self._decoder = None
        self._learned_bags: set = set()       # keys not declared as sequences that a request showed to hold several values
        self._buckets: Dict[int, _Bucket] = {}
        self.graphs_dropped_by: Optional[str] = None     # the feature whose several values made serve() drop the compiled graphs
        self.ragged_overflows = 0             # chunks whose decoded bags exceeded their bucket's capacity: served eagerly
        self._compiled_with: Optional[dict] = None       # compile()'s arguments
        self._recompile = False               # a request showed a new bag that the compiled ragged capacity serves

    @property
    def compiled_buckets(self) -> List[int]:
        """The bucket sizes serve() has a captured graph for right now: empty before compile(), and again after a request
        turned a column into a bag (`graphs_dropped_by` names it; a process that watches this sees the downgrade)."""
        return sorted(self._buckets)

    def tower_buckets(self) -> List[int]:
        """the buckets whose captured graph holds the fused tower's launch"""
        return sorted(size for size, b in self._buckets.items() if b.tower)

    def predict(self, serialized_examples: Sequence[bytes]) -> Dict[str, np.ndarray]:
        from .estimator import ModeKeys
        est = self.estimator
        features = self.receiver(serialized_examples)
        features, _ = est._to_device(features, None)
        self._ensure_loaded(features)
        spec = est._call_model_fn(features, None, ModeKeys.PREDICT)
        return {k: v.detach().cpu().numpy() for k, v in spec.predictions.items()}

    def _ensure_loaded(self, features) -> None:
        from .estimator import ModeKeys
        if not self._loaded:
            self.estimator._build(features, None, ModeKeys.PREDICT)
            self.estimator.load_variables(self._variables)
            self._loaded, self._variables = True, None

    # ---- the native decoder: what the receiver's feature spec asks for, described by the model's own columns -------------------
    def _layout(self):
        """-> (single-valued id keys, bag keys, float keys [(key, shape, n, default)]), each in sorted key order"""
        from .feature_column import CategoricalColumn
        cols = _columns_by_key(self.estimator.params)
        ids, bags, floats = [], [], []
        for key in sorted(self.feature_spec):
            sp = self.feature_spec[key]
            if sp[0] == "fixed":
                floats.append((key, tuple(sp[2]), int(np.prod(sp[2])), sp[3]))
                continue
            col = cols.get(key)
            if not isinstance(col, CategoricalColumn) or not col.vocabulary_file:
                raise NotImplementedError(f"serve: the native decoder needs a vocabulary-file column for feature {key!r} "
                                          "(predict() decodes anything the receiver's spec describes)")
            (bags if (col.is_sequence or key in self._learned_bags) else ids).append((key, col))
        return ids, bags, floats

    def ragged_keys(self) -> List[str]:
        """The features that reach the model as a Ragged (bags, histories): declared sequences, and keys a request showed to
        hold several values.  A model with any is compiled only with compile(ragged_capacity=); without it, it is served eagerly."""
        return [k for k, _ in self._layout()[1]]

    def _open_decoder(self):
        from .io import native
        if self._decoder is None:
            ids, bags, floats = self._layout()
            dec = native.ExampleDecoder([(k, c.vocabulary_file) for k, c in ids], [(k, c.vocabulary_file) for k, c in bags],
                                        [(k, n, d) for k, _, n, d in floats])
            self._decoder = (dec, ids, bags, floats)
        return self._decoder

    @staticmethod
    def _span_bytes(rows: int, F: int, NF: int):
        """the staging / static-input layout of `rows` rows: [ids int64 [rows, F] | pad to 16 bytes | floats float32 [rows, NF]]"""
        id_bytes = (rows * F * 8 + 15) // 16 * 16
        return id_bytes, id_bytes + max(rows * NF * 4, 16)

    def _views(self, span, rows: int, caps=None):
        """the feature dict over a uint8 span of that layout (host or device): id columns of one matrix, float blocks of another;
        `caps` (ragged_span_layout): a Ragged of fixed capacity per bag / history key"""
        import torch
        _, ids, _, floats = self._open_decoder()
        F, NF = len(ids), sum(n for _, _, n, _ in floats)
        id_bytes, _ = self._span_bytes(rows, F, NF)
        feats = {}
        if F:
            mat = span[:rows * F * 8].view(torch.int64).view(rows, F)
            feats.update({k: mat[:, j] for j, (k, _) in enumerate(ids)})
        if NF:
            fmat = span[id_bytes:id_bytes + rows * NF * 4].view(torch.float32).view(rows, NF)
            off = 0
            for k, shape, n, _ in floats:
                feats[k] = fmat[:, off:off + n].view((rows,) + shape)
                off += n
        if caps:
            from .feature_column import Ragged
            for k, (off_at, val_at, cap) in ragged_span_layout(rows, F, NF, caps)[0].items():
                feats[k] = Ragged(span[val_at:val_at + cap * 8].view(torch.int64), span[off_at:off_at + (rows + 1) * 8].view(torch.int64))
        return feats

    def _decode_to(self, records, rows: int, dst=None, caps=None):
        """Decodes `records` (at most `rows`) into pinned staging of the `rows`-row layout — the rows past the request padded with
        id -1 / 0.0 — and moves it with ONE copy: into `dst` (a bucket's static span), or to a new device span.
        -> (device span, {bag key: (offsets, values)})
        `caps` (a bucket compiled with a ragged capacity): the bags go into the span's ragged pieces too, the rows past the
        request as empty bags; a bag that does not fit leaves them empty and the returned dict holds "__overflow__": True."""
        import torch
        from .io.native import SeveralValues
        est = self.estimator
        while True:
            dec, ids, bags, floats = self._open_decoder()
            F, NF, n = len(ids), sum(k[2] for k in floats), len(records)
            id_bytes, total = self._span_bytes(rows, F, NF)
            pieces = None
            if caps:
                pieces, total = ragged_span_layout(rows, F, NF, caps)
            got = {}

            def fill(buf, dec=dec, F=F, NF=NF, n=n, id_bytes=id_bytes, pieces=pieces):
                host = buf.numpy()
                mat = host[:rows * F * 8].view(np.int64).reshape(rows, F)
                fmat = host[id_bytes:id_bytes + rows * NF * 4].view(np.float32).reshape(rows, NF)
                got["bags"] = dec.decode(records, ids=mat[:n], floats=fmat[:n], threads=self.DECODE_THREADS if n >= 256 else 0)[2]
                mat[n:] = -1
                fmat[n:] = 0.0
                if pieces and not _fill_ragged_pieces(host, pieces, got["bags"], rows, n):
                    got["bags"] = dict(got["bags"], __overflow__=True)
            try:
                if est.device.type != "cuda":
                    buf = torch.empty(total, dtype=torch.uint8)
                    fill(buf)
                    return buf, got["bags"]
                return est._h2d(fill, (total,), torch.uint8, dst=dst), got["bags"]
            except SeveralValues as e:
                # a column that is not declared a sequence holds several values: from now on it is decoded as a bag, and a
                # model with a bag is not served from captured graphs (compile() says so)
                if e.key is None or e.key in self._learned_bags:
                    raise
                import warnings
                self._learned_bags.add(e.key)
                self._decoder = None
                cap = (self._compiled_with or {}).get("ragged_capacity")
                if self._buckets and cap is not None and (not isinstance(cap, dict) or e.key in cap):
                    # compiled with a ragged capacity that serves this key: serve() captures the buckets again, the key a bag
                    self._buckets, self._recompile = {}, True
                elif self._buckets:
                    warnings.warn(f"serve: feature {e.key!r} holds several values in a record; the compiled graphs are dropped "
                                  "and requests are served eagerly")
                    self._buckets, self.graphs_dropped_by = {}, e.key
                dst = None

    def _ragged_features(self, bags, n: int):
        """{key: Ragged | dense ids} of the decoded bags, as CategoricalColumn.ids presents a parsed request: a column that is not
        a sequence and holds at most one value per row in THIS request is a dense [n] id vector (-1 where it has none)."""
        import torch
        from .feature_column import Ragged
        dev, out = self.estimator.device, {}
        cols = {k: c for k, c in self._open_decoder()[2]}
        for key, (offsets, values) in bags.items():
            lens = np.diff(offsets)
            if not cols[key].is_sequence and n > 0 and int(lens.max()) <= 1:
                dense = np.full(n, -1, dtype=np.int64)
                dense[lens == 1] = values
                out[key] = torch.from_numpy(dense).to(dev)
            else:
                out[key] = Ragged(torch.from_numpy(np.ascontiguousarray(values)).to(dev), torch.from_numpy(offsets.copy()).to(dev))
        return out

    # ---- serving ----------------------------------------------------------------------------------------------------------------
    def serve(self, serialized_examples: Sequence[bytes]) -> Dict[str, np.ndarray]:
        """predict()'s contract on the native decoder: the compiled graph of the request's bucket when compile() has run (a
        request larger than the largest bucket in chunks), the eager PREDICT model_fn otherwise."""
        records = list(serialized_examples)
        n = len(records)
        while n > 0:
            if self._recompile:
                # a column showed several values for the first time and compile() was given a capacity that serves it: the
                # buckets are captured again with the column as a bag (once per such column, not per request)
                self._recompile = False
                self.compile(**self._compiled_with)
            if not self._buckets:
                break
            out = self._serve_compiled(records)
            if out is not None:
                return out
            if not self._recompile:
                break
        return self._serve_eager(records)

    def _serve_compiled(self, records):
        """the request through the captured graphs, or None when decoding it dropped them"""
        parts = []
        for at, rows, size in plan_chunks(len(records), list(self._buckets)):
            if not self._buckets:                 # (a request that turned a column into a bag dropped the graphs)
                return None
            b = self._buckets[size]
            _, bags = self._decode_to(records[at:at + rows], size, dst=b.span, caps=b.caps)
            if not self._buckets:
                return None
            if bags.get("__overflow__"):
                # a bag larger than the bucket's capacity is never truncated: this chunk runs eagerly (the same kernels)
                self.ragged_overflows += 1
                parts.append(self._serve_eager(records[at:at + rows]))
                continue
            b.graph.replay()
            parts.append({k: v[:rows].cpu().numpy() for k, v in b.out.items()})
        return {k: (np.concatenate([p[k] for p in parts]) if len(parts) > 1 else parts[0][k]) for k in parts[0]}

    def _serve_eager(self, records) -> Dict[str, np.ndarray]:
        """native decode, then the eager PREDICT model_fn"""
        import torch
        from .estimator import ModeKeys
        n = len(records)
        with torch.no_grad():
            span, bags = self._decode_to(records, n)
            features = self._views(span, n)
            features.update(self._ragged_features(bags, n))
            self._ensure_loaded(features)
            spec = self.estimator._call_model_fn(features, None, ModeKeys.PREDICT)
        return {k: v.detach().cpu().numpy() for k, v in spec.predictions.items()}

    def _ragged_caps(self, ragged_capacity):
        """[(bag / history key, values per row)] in decoder order for compile(ragged_capacity=): an int for every key, or a dict
        that names each.  A history additionally needs a static number of steps: NotImplementedError names the parameter."""
        from .estimator import check_ragged_capacity
        policy = check_ragged_capacity(ragged_capacity)
        if policy == "auto":
            raise ValueError("compile: ragged_capacity is an int or a dict of values per row (serving sees no warm-up batches "
                             "to size 'auto' from)")
        _, _, bags, _ = self._open_decoder()
        params = self.estimator.params
        if any(c.is_sequence for _, c in bags):
            static_T = params.get("static_sequence_length") if "static_sequence_length" in params else params.get("sequence_max_length")
            if not static_T:
                name = "static_sequence_length" if "static_sequence_length" in params else "sequence_max_length"
                raise NotImplementedError(f"compile: a model with a history needs a static number of steps: set params[{name!r}] "
                                          "(sequence_max_length: DIN, DIEN; static_sequence_length: BST)")
        caps = []
        for key, _ in bags:
            cap = policy.get(key) if isinstance(policy, dict) else policy
            if cap is None:
                raise ValueError(f"compile: ragged_capacity names no capacity for the ragged feature {key!r}")
            caps.append((key, int(cap)))
        return caps

    def compile(self, batch_sizes: Sequence[int] = (1, 16, 64, 256, 1024, 4096), warmup: int = 2,
                ragged_capacity=None) -> "ServingModel":
        """Captures the PREDICT model_fn once per bucket size into a torch.cuda.CUDAGraph over private static inputs (one stream,
        no forked branch; warm-up on a side stream, then capture_error_mode="thread_local", as estimator.GraphedTrainStep).
        Under the capture the VariableStore's serving switch is on: buckets of at most nn.SERVE_TOWER_MAX_ROWS rows run their
        hidden stack as ONE launch with the BatchNorms folded (nn.LazyTower); the folds are computed here, once.
        A model whose decoded features contain a Ragged (a bag, a history) is compiled only with `ragged_capacity`, values per row
        as an int or a dict key -> int: a bucket's span then holds offsets [rows + 1] and values [rows * capacity] per such key
        (ragged_span_layout), and a chunk whose bags do not fit is served eagerly (ragged_overflows).  Without it
        NotImplementedError names the keys; serve() still serves the model (native decode, eager model_fn).  A model whose
        launches depend on the request's data even then (a history without a static length) is refused the same way."""
        import torch
        from . import nn
        from .estimator import ModeKeys
        est = self.estimator
        sizes = sorted({int(b) for b in batch_sizes})
        if not sizes or sizes[0] < 1:
            raise ValueError(f"compile: batch_sizes must be positive, got {list(batch_sizes)}")
        ragged = self.ragged_keys()
        if ragged and ragged_capacity is None:
            raise NotImplementedError("compile: the decoded features " + ", ".join(ragged) + " are ragged (bags / histories); pass "
                                      "ragged_capacity= (values per row) to capture graphs over fixed-capacity buffers — serve() "
                                      "serves this model eagerly")
        caps = self._ragged_caps(ragged_capacity)
        if est.device.type != "cuda":
            raise RuntimeError("compile: captured graphs need a HIP device")
        _, ids, _, floats = self._open_decoder()
        F, NF = len(ids), sum(k[2] for k in floats)
        folds = None
        buckets: Dict[int, _Bucket] = {}
        with torch.no_grad():
            for size in sizes:
                b = _Bucket()
                b.rows, b.caps = size, caps
                total = ragged_span_layout(size, F, NF, caps)[1] if caps else self._span_bytes(size, F, NF)[1]
                b.span = torch.zeros(total, dtype=torch.uint8, device=est.device)
                b.features = self._views(b.span, size, caps)
                if F:
                    b.span[:size * F * 8].view(torch.int64).fill_(-1)          # (a bucket of padding rows: id -1, 0.0)
                for k, _ in caps or ():
                    b.features[k].values.fill_(-1)                            # (... and empty bags: offsets 0, values -1)
                self._ensure_loaded(b.features)
                est.store.data_dependent = None
                if folds is None:
                    folds = fold_batch_norms(est.store.named_arrays())
                plan = nn.ServingPlan(nn.SERVE_TOWER_MAX_ROWS, folds, nn.BN_EPSILON)

                def run(b=b, plan=plan):
                    est.store.serving = plan
                    try:
                        return dict(est._call_model_fn(b.features, None, ModeKeys.PREDICT).predictions)
                    finally:
                        est.store.serving = None
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(max(int(warmup), 1)):
                        run()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                if caps and est.store.data_dependent:    # (said by the warm-up runs: never found out inside a capture)
                    raise NotImplementedError(f"compile: the model is not capturable over ragged inputs: {est.store.data_dependent}")
                b.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(b.graph, capture_error_mode="thread_local"):
                    b.out = run()
                b.tower = plan.tower_launches > 0          # (whether the captured graph holds the fused tower's launch)
                b.plan = plan                     # (the captured launches read the folds: they live as long as the graph)
                buckets[size] = b
        self._buckets = buckets
        self._compiled_with = dict(batch_sizes=tuple(sizes), warmup=warmup, ragged_capacity=ragged_capacity)
        return self
