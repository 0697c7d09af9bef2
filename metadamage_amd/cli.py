"""`metadamage` command line (mirror of /root/reference/metadamage/cli.py).

Same sub-command and flags as the reference's `metadamage fit` (cli.py:97-159)
so existing invocations keep working; `--version` as cli.py:72-77.  The
`dashboard` sub-command is out of scope (the reference's Dash viewer reads the
parquet files this writes unchanged); it reports that and exits non-zero.
"""

from __future__ import annotations

import logging
from pathlib import Path
from typing import List, Optional

import typer

from . import utils
from .__version__ import __version__
from .main import main

out_dir_default = Path("./data/out/")

cli_app = typer.Typer(add_completion=False)


def version_callback(value: bool):
    if value:
        typer.echo(f"Metadamage CLI, version: {__version__}")
        raise typer.Exit()


@cli_app.callback()
def callback(version: Optional[bool] = typer.Option(None, "--version", callback=version_callback)):
    """
    Metagenomics Ancient Damage: metadamage (MI355X engine).

    Run the fit command:

    \b
        $ metadamage fit --help
    """


@cli_app.command("fit")
def cli_fit(
    filenames: List[Path] = typer.Argument(...),
    out_dir: Path = typer.Option(out_dir_default),
    max_fits: Optional[int] = typer.Option(None, help="[default: None (All fits)]"),
    max_cores: int = 1,
    min_alignments: int = 10,
    min_y_sum: int = 10,
    substitution_bases_forward: utils.SubstitutionBases = typer.Option(utils.SubstitutionBases.CT),
    substitution_bases_reverse: utils.SubstitutionBases = typer.Option(utils.SubstitutionBases.GA),
    forced: bool = typer.Option(False, "--forced"),
    inference: str = typer.Option("nuts", help="nuts: NUTS sampling as the reference; map: MAP fit; "
                                  "map-laplace: MAP fit with Laplace standard errors and significance; "
                                  "nuts-diag: NUTS with per-chain ESS, split R-hat, MCSE and divergences; "
                                  "nuts-summary: NUTS with posterior std, median, 68 % HPDI and significance; "
                                  "nuts-loo: NUTS with PSIS-LOO model comparison and Pareto-k diagnostics; "
                                  "map-psis: MAP fit with an importance-sampled posterior and its Pareto-k; "
                                  "map-waic: MAP fit with importance-weighted WAIC n_sigma and asymmetry; "
                                  "map-evidence: MAP fit with the importance-sampled evidence of the damage and "
                                  "null models, their Bayes factor and the probability of damage; "
                                  "map-pred: MAP fit with the importance-weighted posterior predictive D_max, its "
                                  "68 % interval and fit_predictions columns; "
                                  "auto: MAP fit with its importance-sampled correction, NUTS only for the taxa "
                                  "whose Pareto-k says it cannot be trusted"),
    psis_draws: int = typer.Option(256, help="map-psis, map-waic, map-evidence, map-pred, auto: importance draws per sub-fit, "
                                   "25 to 1024"),
    pred_draws: int = typer.Option(1000, help="map-pred, auto with --auto-pred: predictive draws per position, 25 to 1024"),
    psis_adapt: int = typer.Option(0, help="map-psis, map-waic, map-evidence, auto: at most this many moment-matched proposal "
                                   "rounds for a sub-fit whose Pareto-k is over the threshold, 0 to 4"),
    auto_pred: bool = typer.Option(False, "--auto-pred", help="auto: D_max, its 68 % interval and the fit_predictions "
                                   "rows of a taxon that is not sampled from the importance-weighted posterior "
                                   "predictive (--pred-draws draws per position)"),
    ppc: bool = typer.Option(False, "--ppc", help="map-pred: the posterior predictive check of the damage model -- "
                             "p-values for an outlying position and for a strand difference, the worst position, "
                             "and a per-position p-value in fit_predictions"),
    quantiles: bool = typer.Option(False, "--quantiles", help="map-psis: the importance-weighted posterior median, "
                                   "68 % HPDI and 5 % / 95 % quantiles of D_max, the median and HPDI of q, the "
                                   "medians of A, c and the concentration, and P(D_max > --dmax-threshold)"),
    dmax_threshold: float = typer.Option(0.01, help="map-psis with --quantiles: the threshold of D_max_prob_above, "
                                         "0 to 1"),
    joint: bool = typer.Option(False, "--joint", help="map-waic: the evidence and Bayes factors of map-evidence and "
                               "the posterior mean and std of map-psis from the same importance weights, in the "
                               "same launch and the same fit_results file"),
):
    """Fitting Ancient Damage.

    FILENAME is the name of the file(s) to fit (with the ancient-model)

    \b
        $ metadamage fit --max-fits 10 --max-cores 2 ./data/input/data_ancient.txt
    """
    logging.basicConfig(level=logging.WARNING, format="%(message)s")
    d_cfg = {
        "out_dir": out_dir,
        "max_fits": max_fits,
        "max_cores": max_cores,
        "min_alignments": min_alignments,
        "min_y_sum": min_y_sum,
        "substitution_bases_forward": substitution_bases_forward.value,
        "substitution_bases_reverse": substitution_bases_reverse.value,
        "forced": forced,
        "version": "0.0.0",
        "inference": inference,
        "psis_draws": psis_draws,
        "pred_draws": pred_draws,
        "psis_adapt": psis_adapt,
        "auto_pred": auto_pred,
        "ppc": ppc,
        "quantiles": quantiles,
        "dmax_threshold": dmax_threshold,
        "joint": joint,
    }
    if inference not in ("nuts", "map", "map-laplace", "map-psis", "map-waic", "map-pred", "map-evidence", "nuts-diag",
                         "nuts-summary", "nuts-loo", "auto"):
        raise typer.BadParameter("--inference must be nuts, map, map-laplace, map-psis, map-waic, map-pred, "
                                 "map-evidence, nuts-diag, nuts-summary, nuts-loo or auto")
    if not 25 <= psis_draws <= 1024:
        raise typer.BadParameter("--psis-draws must be in [25, 1024]")
    if not 25 <= pred_draws <= 1024:
        raise typer.BadParameter("--pred-draws must be in [25, 1024]")
    if not 0 <= psis_adapt <= 4:
        raise typer.BadParameter("--psis-adapt must be in [0, 4]")
    if psis_adapt and inference not in ("map-psis", "map-waic", "map-evidence", "auto"):
        raise typer.BadParameter("--psis-adapt goes with --inference map-psis, map-waic, map-evidence or auto")
    if auto_pred and inference != "auto":
        raise typer.BadParameter("--auto-pred goes with --inference auto")
    if ppc and inference != "map-pred":
        raise typer.BadParameter("--ppc goes with --inference map-pred")
    if quantiles and inference != "map-psis":
        raise typer.BadParameter("--quantiles goes with --inference map-psis")
    if joint and inference != "map-waic":
        raise typer.BadParameter("--joint goes with --inference map-waic")
    if not 0.0 <= dmax_threshold <= 1.0:
        raise typer.BadParameter("--dmax-threshold must be in [0, 1]")
    cfg = utils.Config(**d_cfg)
    cfg.add_filenames(filenames)
    # launched by torchrun (WORLD_SIZE > 1): one rank per GPU, the rank's GPU
    # selected before any device call, RCCL process group; main() then deals
    # files or shards taxa over the ranks and rank 0 writes the shared results
    from .distributed import run_distributed

    run_distributed(main, filenames, cfg)


@cli_app.command("dashboard")
def cli_dashboard(dir: Path = typer.Argument(out_dir_default), debug: bool = typer.Option(False, "--debug")):
    """Dashboard: not part of this engine (the reference dashboard reads its output as-is)."""
    typer.echo("The dashboard is not part of metadamage_amd; run the reference `metadamage dashboard "
               f"{dir}` on the output directory.")
    raise typer.Exit(code=2)


def cli_main():
    cli_app(prog_name="metadamage")
