"""Which steps of a fused call are samples, and the parts of a request that every statistic of the record ring parses alike.

A request (``PCTrainer.mcpc_moments``, ``mcpc_covariance``, ...) is a dict; its ``begin`` and ``stride`` name the steps of the call whose
records are samples.  ``SampleWindow`` is the one definition of that set and of how it falls into the slices of a call; the ``parse_*``
functions below are the one copy of the checks the request modules share.  Every function takes the request's name (``"mcpc_moments"``)
so that an error says whose request it is.  Where the requests differ in what they accept, the difference is an argument here, set by
the module that wants it.  No device code, and nothing of torch.
"""
from dataclasses import dataclass
from typing import List


def sample_steps(begin: int, T: int, stride: int) -> range:
    """The steps of a call of T steps whose records are samples."""
    return range(begin, T, stride)


def human_bytes(n: int) -> str:
    for unit, size in (("GiB", 1 << 30), ("MiB", 1 << 20), ("KiB", 1 << 10)):
        if n >= size:
            return f"{n / size:.1f} {unit}"
    return f"{n} B"


@dataclass(frozen=True)
class SampleWindow:
    """The samples of a call of ``T`` steps: steps ``begin, begin + stride, ...`` below ``T``.  The base of every ``*Spec``."""
    begin: int
    stride: int
    T: int

    @property
    def n(self) -> int:
        return len(sample_steps(self.begin, self.T, self.stride))

    @property
    def steps(self) -> List[int]:
        return list(sample_steps(self.begin, self.T, self.stride))

    def chunk(self, t0: int, n_steps: int):
        """(first, count): the samples among steps t0 .. t0 + n_steps - 1 are rows first, first + stride, ... of a chunk that holds
        one record per step from t0 on."""
        f = self.begin if t0 <= self.begin else self.begin + -(-(t0 - self.begin) // self.stride) * self.stride
        return f - t0, len(range(f, min(t0 + n_steps, self.T), self.stride))


def parse_keys(name: str, spec, keys) -> None:
    """``spec`` is a dict with no key outside ``keys``."""
    if not isinstance(spec, dict):
        raise ValueError(f"{name}: expected a dict or None, got {type(spec).__name__}")
    unknown = sorted(k for k in spec if k not in keys)
    if unknown:
        raise ValueError(f"{name}: unknown keys {unknown}; known: {list(keys)}")


def parse_window(name: str, spec, T: int, more_ints=()):
    """(begin, stride, *more): ``begin`` in [0, T), ``stride`` >= 1, defaults 0 and 1.  ``more_ints``: (key, default) of further ints of
    the request whose TYPE is checked together with theirs, before any range (``mcpc_rolling``'s ``every``); their range is the caller's."""
    values = [("begin", spec.get("begin", 0)), ("stride", spec.get("stride", 1))] + [(k, spec.get(k, d)) for k, d in more_ints]
    for key, v in values:
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name}: {key} must be an int, got {v!r}")
    begin, stride = values[0][1], values[1][1]
    if not 0 <= begin < T:
        raise ValueError(f"{name}: begin={begin} outside [0, T={T})")
    if stride < 1:
        raise ValueError(f"{name}: stride={stride}, must be at least 1")
    return tuple(v for _, v in values)


def parse_layers(name: str, spec, n_layers: int, none_means="error"):
    """``layers``: a sequence of layer indices or one int -> sorted, distinct tuple.  ``none_means`` is where the requests differ:
    "error": a missing key is ``()`` and ``layers=None`` is refused as no sequence (moments, errors); "empty": both are ``()``
    (histogram, autocovariance, rolling); "all": both are every latent layer (covariance)."""
    layers = spec.get("layers", None if none_means == "all" else ())
    if layers is None and none_means != "error":
        layers = tuple(range(n_layers)) if none_means == "all" else ()
    if isinstance(layers, int) and not isinstance(layers, bool):
        layers = (layers,)
    try:
        layers = tuple(layers)
    except TypeError:
        raise ValueError(f"{name}: layers must be a sequence of layer indices, got {layers!r}") from None
    for l in layers:
        check_layer_index(name, l, n_layers)
    return tuple(sorted(set(layers)))


def check_layer_index(name: str, l, n_layers: int) -> None:
    if isinstance(l, bool) or not isinstance(l, int) or not 0 <= l < n_layers:
        raise ValueError(f"{name}: layer index {l!r} out of range, the model has {n_layers} PC layers (0..{n_layers - 1})")


def parse_layer(name: str, spec, n_layers: int, role: str) -> int:
    """``layer``: the one required layer of a request; ``role`` finishes the sentence "the PC layer ..."."""
    if "layer" not in spec or spec["layer"] is None:
        raise ValueError(f"{name}: layer is required: the PC layer {role}, an int in 0..{n_layers - 1}")
    layer = spec["layer"]
    if isinstance(layer, bool) or not isinstance(layer, int):
        raise ValueError(f"{name}: layer must be an int, got {layer!r}")
    check_layer_index(name, layer, n_layers)
    return layer


def parse_outputs(name: str, spec, n_out: int, allowed=(None, "identity", "sigmoid")):
    """``outputs``: one of ``allowed`` (the first is None, the default), and a read-out to take it from."""
    outputs = spec.get("outputs", None)
    if outputs not in allowed:
        raise ValueError(f"{name}: outputs={outputs!r}, expected None, {allowed[1]!r} or {allowed[2]!r}")
    if outputs is not None and n_out < 1:
        raise ValueError(f"{name}: outputs asked of a model without a read-out (it ends with a PCLayer)")
    return outputs


def require_columns(name: str, layers, outputs) -> None:
    if not layers and outputs is None:
        raise ValueError(f"{name}: no columns: layers is empty and outputs is None")


def column_list(layers, sizes, out_name, n_out: int, layer_name="x{}".format, starts=False):
    """The blocks of a request in order: ``(name, width)`` per layer, then the read-out's if ``out_name`` is not None; with ``starts``
    ``(name, start, width)``, the start being the block's first column among all of them."""
    cols = [(layer_name(l), int(sizes[l])) for l in layers] + ([(out_name, int(n_out))] if out_name is not None else [])
    if not starts:
        return tuple(cols)
    out, start = [], 0
    for nm, w in cols:
        out.append((nm, start, w))
        start += w
    return tuple(out)


def slice_bounds(T: int, S: int, keep=None):
    """[(t0, n), ...]: a call of ``T`` steps as consecutive slices of at most ``S`` steps.  ``keep = (a, b)``: no slice ends strictly
    inside steps a .. b - 1 (the window that accumulates parameter gradients stays in ONE slice, however long): a slice that would
    is cut at ``a`` if it starts before it, and runs to ``b`` otherwise."""
    bounds, t0 = [], 0
    while t0 < T:
        n = min(S, T - t0)
        if keep is not None and keep[0] < t0 + n < keep[1]:              # it would end inside the window
            n = keep[0] - t0 if t0 < keep[0] else keep[1] - t0
        bounds.append((t0, n))
        t0 += n
    return bounds
