"""The optional post-fit blocks and the tails that ride them, two tables.

A run carries at most one block of BLOCKS and, behind it, the tails of TAILS
that ride it.  The order base record (out, pred, status) | block | ppc | quant |
joint | auto_pred | adapt is decided here once: it is TAILS' order, and the
gather record (distributed), the returned tuples (engine) and the frames'
keywords (fits) all walk Run.parts.  describe() turns what a caller asks for
into that one Run and makes every check on the way; no layer re-checks.

A new block costs one entry in BLOCKS, one launch function in engine._LAUNCH
and its columns in fits.make_df_fit_results.  A new tail costs one entry in
TAILS (its option, its switch, the blocks it rides, its shapes and its two
refusals), one launch function in engine._LAUNCH unless its block's launch
writes it, its keyword on the public entry points that take it, and its columns
in fits.make_df_fit_results.  The buffers, the rounding copy, the transfers, the
chunk plan's bytes, the gather record's offsets and the order of the returned
arrays follow from the entry.
"""

from __future__ import annotations

from dataclasses import dataclass
from math import prod

from . import _lib


class _Part:
    """What a block and a tail share: f32 `shape` per taxon on the way out, `device` pieces as computed."""

    @property
    def out_bytes(self) -> int:
        return 4 * prod(self.shape)

    @property
    def device_bytes(self) -> int:
        return sum(prod(shape) * (8 if dtype == "float64" else 4) for shape, dtype in self.device)


@dataclass(frozen=True)
class Block(_Part):
    name: str  # the keyword of fits.fit_packed and engine.fit_batch_host
    inference: str  # the --inference value that asks for it
    mode: int | None  # the opts.mode it needs (None: auto runs both fits)
    attr: str  # its attribute on engine.FitBatch and distributed.Records
    shape: tuple  # f32 per taxon as it leaves the device (the gather record, the host arrays)
    device: tuple = ()  # ((shape, dtype), ...) per taxon as the launch computes it
    sampled: bool = False  # importance-sampled: takes psis_draws and psis_adapt (and then the adapt tail)
    chunked: bool = True  # engine.ChunkedFitter runs it (auto: engine.fit_auto_chunks does; a layout entry only)

    @property
    def switch(self) -> str:  # its keyword in engine and distributed
        return "with_" + self.name


def _f64(*shape):
    """shape, device of a block the launch writes as float64 and the dispatch rounds to f32 in place."""
    return {"shape": shape, "device": ((shape, "float64"),)}


BLOCKS = (
    # the Laplace standard errors of the three PMD sub-fits (_lib.LAPLACE_FIELDS)
    Block("laplace", "map-laplace", _lib.MODE_MAP, "lap", **_f64(3, _lib.NLAPLACE)),
    # the sampling diagnostics of the six sub-fits (_lib.NUTSDIAG_FIELDS).  On the way out a row's flags are valid +
    # 2 * the chain's divergence count (the record's diagnostic slot 7, which does not leave the device otherwise)
    Block("diag", "nuts-diag", _lib.MODE_NUTS, "diag", **_f64(_lib.NSUBFIT, _lib.NNUTSDIAG)),
    # the posterior summaries of the six sub-fits (_lib.NUTSSUMM_FIELDS)
    Block("summary", "nuts-summary", _lib.MODE_NUTS, "summ", **_f64(_lib.NSUBFIT, _lib.NNUTSSUMM)),
    # the PSIS-LOO records, row 6 the comparisons (_lib.NUTSLOO_FIELDS, _lib.NUTSLOO_COMPARE_FIELDS)
    Block("loo", "nuts-loo", _lib.MODE_NUTS, "loo", **_f64(_lib.NLOOROW, _lib.NNUTSLOO)),
    # the importance-sampled posteriors of the three PMD sub-fits (_lib.MAPPSIS_FIELDS)
    Block("psis", "map-psis", _lib.MODE_MAP, "psis", **_f64(3, _lib.NMAPPSIS), sampled=True),
    # the importance-weighted WAIC records, row 6 the comparisons (_lib.MAPWAIC_FIELDS, _lib.MAPWAIC_COMPARE_FIELDS)
    Block("waic", "map-waic", _lib.MODE_MAP, "waic", **_f64(_lib.NWAICROW, _lib.NMAPWAIC), sampled=True),
    # the importance-sampled evidence records, row 6 the Bayes factors (_lib.MAPEVID_FIELDS,
    # _lib.MAPEVID_COMPARE_FIELDS)
    Block("evidence", "map-evidence", _lib.MODE_MAP, "evid", **_f64(_lib.NEVIDROW, _lib.NMAPEVID), sampled=True),
    # the posterior predictive: computed as f32 predictions [3][30] and an f64 record (_lib.MAPPRED_FIELDS), out as
    # one f32 block ppred | rec (engine.split_ppred); also takes pred_draws
    Block("ppred", "map-pred", _lib.MODE_MAP, "ppred", (_lib.NPRED * _lib.NPOS + _lib.NMAPPRED,),
          (((_lib.NPRED, _lib.NPOS), "float32"), ((_lib.NMAPPRED,), "float64")), sampled=True),
    # route, sampled, khat_max, ess_min of the auto inference
    Block("auto", "auto", None, "auto", (_lib.NAUTO,), sampled=True, chunked=False),
)
_BY_NAME = {b.name: b for b in BLOCKS}


@dataclass(frozen=True)
class Tail(_Part):
    name: str  # its attribute on engine.FitBatch and distributed.Records, its keyword of fits.make_df_fit_results
    option: str  # the option of fits.fit_packed and the engine that asks for it
    switch: str  # its keyword in distributed
    rides: tuple  # the names of the blocks it may ride with
    shape: tuple  # f32 per taxon as it leaves the device
    device: tuple  # ((shape, dtype), ...) per taxon as the launch computes it (): fit_auto_device forms it)
    refusal: str  # the ValueError of an option without a block it rides
    switch_refusal: str  # ... and of its switch in distributed
    block_switches: tuple = ()  # ((block name, switch), ...): the blocks that ask for it by a switch of their own

    attr = property(lambda self: self.name)


TAILS = (
    # the posterior predictive check, ppos | rec (_lib.MAPPPC_FIELDS; engine.split_ppc)
    Tail("ppc", "ppc", "with_ppc", ("ppred",), (_lib.NPPCOUT,),
         (((_lib.NPOS,), "float32"), ((_lib.NMAPPPC,), "float64")),
         "ppc needs with_ppred: the check is of the predictive that mdfit_map_pred forms",
         "with_ppc goes with with_ppred"),
    # the weighted order statistics of the three PMD rows (_lib.MAPQUANT_FIELDS); also takes dmax_threshold
    Tail("quant", "quantiles", "with_quant", ("psis",), (_lib.NQUANTOUT,), (((3, _lib.NMAPQUANT), "float64"),),
         "quantiles needs with_psis: the order statistics are of the posterior mdfit_map_psis forms",
         "with_quant goes with with_psis"),
    # the fused launch's other two records, evid | psis (engine.split_joint)
    Tail("joint", "joint", "with_joint", ("waic",), (_lib.NJOINTOUT,),
         (((_lib.NEVIDROW, _lib.NMAPEVID), "float64"), ((3, _lib.NMAPPSIS), "float64")),
         "joint needs with_waic: mdfit_map_joint writes the evidence and the posterior beside the waic record",
         "with_joint goes with with_waic"),
    # pred_ess_min, pred_distinct_min of the auto inference's predictive
    Tail("auto_pred", "auto_pred", "with_auto_pred", ("auto",), (_lib.NAUTOPRED,), (),
         "auto_pred goes with the auto inference", "with_auto_pred goes with with_auto"),
    # the rounds' record (_lib.MAPADAPT_FIELDS), out as the two columns of engine.adapt_summary; its option is the
    # round cap, an integer.  It rides the sampled blocks; the ppred block asks for it by a switch of its own
    Tail("adapt", "psis_adapt", "with_adapt", tuple(b.name for b in BLOCKS if b.sampled), (_lib.NADAPTOUT,),
         (((3, _lib.NMAPADAPT), "float64"),),
         "psis_adapt needs with_psis, with_waic, with_ppred or the auto inference",
         "with_adapt goes with with_psis, with_waic or with_auto", (("ppred", "with_ppred_adapt"),)),
)
ADAPT = TAILS[-1]  # the tail whose option is a count


def select(**switches) -> Block | None:
    """The run's one block from the with_* switches (None: no block)."""
    unknown = sorted(set(switches) - {b.switch for b in BLOCKS})
    if unknown:
        raise TypeError(f"unknown block switch {', '.join(unknown)}: the switches are "
                        + ", ".join(b.switch for b in BLOCKS))
    on = [b for b in BLOCKS if switches.get(b.switch)]
    if len(on) > 1:
        raise ValueError(" and ".join(b.switch for b in on) + " are mutually exclusive: one extra block per run")
    return on[0] if on else None


def resolve(opts, **switches) -> Block | None:
    """select, and the block's mode checked against opts.mode (opts None: the default options, MAP)."""
    block = select(**switches)
    if block is not None and block.mode is not None:
        mode = _lib.MODE_MAP if opts is None else int(opts.mode)
        if mode != block.mode and block.mode == _lib.MODE_MAP:
            raise ValueError(f"{block.switch} needs MAP records (opts.mode == MODE_MAP)")
        if mode != block.mode:
            raise ValueError(f"{block.switch} needs the chains of a sampling call (opts.mode == MODE_NUTS)")
    return block


def check_rounds(psis_adapt: int, rides: bool) -> int:
    """The round cap of MDFIT-ADAPT v1: 0 .. ADAPT_MAX_ROUNDS and, when not 0, with a block the adapt tail rides."""
    R = int(psis_adapt)
    if not 0 <= R <= _lib.ADAPT_MAX_ROUNDS:
        raise ValueError(f"psis_adapt must be in [0, {_lib.ADAPT_MAX_ROUNDS}]")
    if R > 0 and not rides:
        raise ValueError(ADAPT.refusal)
    return R


@dataclass(frozen=True)
class Run:
    """One run as every layer reads it."""

    block: Block | None
    tails: tuple  # the active tails, in TAILS' order
    psis_draws: int
    pred_draws: int | None
    rounds: int  # psis_adapt (a layout of distributed, which has no options: 1 with the adapt tail)
    dmax_threshold: float

    @property
    def parts(self) -> tuple:
        """[block, *tails]: what follows the base record, in the record's order."""
        return ((self.block,) if self.block is not None else ()) + self.tails

    def has(self, name: str) -> bool:
        return any(t.name == name for t in self.tails)

    def option(self, tail: Tail):
        """The tail's option as the engine takes it."""
        return self.rounds if tail is ADAPT else self.has(tail.name)

    @property
    def key(self) -> tuple:
        """What tells two runs' buffers apart (engine.staging caches on it): the draw counts only where the block
        uses them, the threshold only with the tail that takes it."""
        b = self.block
        return (b.name if b is not None else None, self.psis_draws if b is not None and b.sampled else 0,
                self.pred_draws if b is not None and b.name == "ppred" else 0, self.rounds,
                tuple(t.name for t in self.tails), self.dmax_threshold if self.has("quant") else None)

    @property
    def layout(self) -> dict:
        """The switches of distributed.Records and unpack_gathered for this run."""
        name = self.block.name if self.block is not None else None
        return {p.switch if isinstance(p, Block) else dict(p.block_switches).get(name, p.switch): True
                for p in self.parts}

    @property
    def options(self) -> dict:
        """The keywords that ask the engine's entry for this run: fit_auto_chunks' for a block that is not chunked,
        else those of staging, ChunkedFitter and fit_batch_host (the block's own keyword is the caller's)."""
        chunked = self.block is None or self.block.chunked
        kw = {"psis_draws": self.psis_draws, "pred_draws": self.pred_draws}
        if chunked:
            kw["dmax_threshold"] = self.dmax_threshold
        kw.update({t.option: self.option(t) for t in TAILS if any(_BY_NAME[b].chunked == chunked for b in t.rides)})
        return kw


def describe(opts=None, tails=None, *, by_switch: bool = False, check_mode: bool = True, chunked: bool = False,
             psis_draws: int = 256, pred_draws: int | None = 1000, dmax_threshold: float = 0.01, **switches) -> Run:
    """The one resolver: what a caller asks for -> the Run, every check made.

    switches: the block's with_* switch.  tails: {option: value} by TAILS' options (engine and fits; psis_adapt is
    the round cap); by_switch (distributed, which has no options): the tails come among switches instead, by theirs.
    check_mode: the block's mode is checked against opts (resolve); chunked: a block that is not the chunked
    dispatch's is refused."""
    asked = dict(switches)
    if by_switch:
        given = {t: bool(asked.pop(t.switch, False)) for t in TAILS}
        own = {(t, b): bool(asked.pop(s, False)) for t in TAILS for b, s in t.block_switches}
    else:
        tails = dict(tails or {})
        given = {t: tails.pop(t.option, False) for t in TAILS}
        if tails:
            raise TypeError(f"unknown tail option {', '.join(sorted(tails))}")
    block = resolve(opts, **asked) if check_mode else select(**asked)
    if chunked and block is not None and not block.chunked:
        raise ValueError(f"{block.switch} is not the chunked dispatch's: fit_auto_chunks runs it")
    name = block.name if block is not None else None
    rounds = 0
    if by_switch:
        for t in TAILS:
            if given[t] and (name not in t.rides or name in dict(t.block_switches)):
                raise ValueError(t.switch_refusal)
            for b, s in t.block_switches:
                if own[t, b] and name != b:
                    raise ValueError(f"{s} goes with with_{b}")
                given[t] = given[t] or own[t, b]
        rounds = int(given[ADAPT])
    else:
        rounds = check_rounds(given[ADAPT], name in ADAPT.rides)
        given[ADAPT] = rounds > 0
        for t in TAILS:
            if given[t] and name not in t.rides:
                raise ValueError(t.refusal)
    run = Run(block, tuple(t for t in TAILS if given[t]), int(psis_draws),
              int(pred_draws) if pred_draws is not None else None, rounds, float(dmax_threshold))
    if run.has("quant") and not 0.0 <= run.dmax_threshold <= 1.0:
        raise ValueError("dmax_threshold must be in [0, 1]")
    return run
