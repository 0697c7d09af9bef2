"""The optional post-fit blocks, one table: a run carries at most one of them.

engine (the chunk plan, the buffers, the chunked dispatch), distributed (the
gather record's layout) and fits (the frames' keywords) read every per-block
fact from BLOCKS; a new block is one more entry here, one launch function in
engine and its columns in fits.make_df_fit_results.  In the gather record and
in the returned tuples the block follows the base record (out, pred, status);
behind it come the tail blocks, which are no entries: ppc (f32 [42], only with
ppred: the posterior predictive check rides with the predictive it checks),
quant (f32 [48], only with psis: the weighted order statistics ride with the
posterior they summarise),
joint (f32 [104] = evid | psis, only with waic: the fused launch's other two
records ride with the waic record whose weights they share),
auto-pred (f32 [2], only with auto), then adapt (f32 [2], psis_adapt > 0 with a
`sampled` block).
"""

from __future__ import annotations

from dataclasses import dataclass
from math import prod

from . import _lib


@dataclass(frozen=True)
class Block:
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

    @property
    def out_bytes(self) -> int:
        return 4 * prod(self.shape)

    @property
    def device_bytes(self) -> int:
        return sum(prod(shape) * (8 if dtype == "float64" else 4) for shape, dtype in self.device)


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


def select(**switches) -> Block | None:
    """The run's one block from the with_* switches (None: no block); distributed, which has no options, stops here."""
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
