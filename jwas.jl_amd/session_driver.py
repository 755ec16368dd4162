"""What the drivers of the block sessions share before their chains start (megatrait.run_megatrait, mtjoint.run_mtjoint,
chains.run_chains): the refusals common to the models with more than 4 traits, the alignment of records and genotypes, and the engine
with its matrices loaded.  Plain functions; every driver keeps its own priors, its own loop and its own session calls.  What they
share of the outputs is in chain_output.py."""
import numpy as np

from .chain_output import resolve_output_ids


def not_false(x):
    """An optional runMCMC argument that was given (the reference's `!= false`)."""
    return not (x is False or x is None)


def refuse_engine(engine, methods, lacks):
    """An engine without the session's methods (lacks(their names) is the message), or one that drives a shard."""
    missing = [m for m in methods if not hasattr(engine, m)]
    if missing:
        raise NotImplementedError(lacks(", ".join(missing)))
    if hasattr(engine, "comm_info") and engine.comm_info()[1] > 1:
        raise NotImplementedError("models with more than 4 traits are not driven from marker or row shards")


def refuse_beyond_four_traits(model, Mi, *, one_pass, annotation_priors, independent_blocks, fast_blocks, heterogeneous_residuals,
                              location_parameters, causal_structure, RRM, single_step_analysis, starting_value):
    """The refusals that megatrait.validate and mtjoint.validate share, in their order.  one_pass: why fast_blocks does not apply."""
    if Mi.annotations is not False:
        raise NotImplementedError("annotations with more than 4 traits stay on the reference")
    if annotation_priors != "host":
        raise NotImplementedError('annotation_priors="device" does not apply to models with more than 4 traits')
    mode = getattr(Mi, "storage_mode", "dense")
    if mode == "stream":
        raise NotImplementedError("storage=:stream with more than 4 traits stays on the reference (dense storage only)")
    if mode == "device":
        raise NotImplementedError("device_genotypes with more than 4 traits is not supported: pass the genotypes through get_genotypes")
    if independent_blocks:
        raise NotImplementedError("independent_blocks with more than 4 traits stays on the reference")
    if fast_blocks is not False:
        raise NotImplementedError(f"fast_blocks with more than 4 traits stays on the reference ({one_pass})")
    if heterogeneous_residuals:
        raise NotImplementedError("heterogeneous_residuals (residual weights) with more than 4 traits stays on the reference")
    if location_parameters == "device":
        raise NotImplementedError('location_parameters="device" with more than 4 traits is not supported: they are sampled on the host')
    if getattr(model, "rndTrmVec", []):
        raise NotImplementedError("set_random effects with more than 4 traits stay on the reference")
    if any(tt != "continuous" for tt in model.traits_type):
        raise NotImplementedError("categorical_trait / censored_trait with more than 4 traits stay on the reference")
    if not_false(causal_structure):
        raise NotImplementedError("causal_structure runs with at most 4 traits on the device")
    if not_false(RRM):
        raise NotImplementedError("RRM runs with one trait; with more than 4 traits it stays on the reference")
    if not_false(single_step_analysis):
        raise NotImplementedError("single_step_analysis with more than 4 traits stays on the reference")
    if Mi.alpha is not False or not_false(starting_value):
        raise NotImplementedError("starting_value (marker or location-parameter starting values) with more than 4 traits stays on the reference")


def phenotype_records(df, traits):
    """(the ID column, the records with string IDs, their phenotypes t x records); a trait without a column raises."""
    idcol = df.columns[0]
    ph = df.copy()
    ph[idcol] = ph[idcol].astype(str)
    for tr in traits:
        if tr not in ph.columns:
            raise ValueError(f"Phenotypes for {tr} are not found in the data.")
    return idcol, ph, np.stack([ph[tr].to_numpy(dtype=np.float64) for tr in traits])


def align_records(model, Mi, idcol, ph, Yall, ftype, outputEBV):
    """input_data_validation.jl:198-294, tools4genotypes.jl:288-323: the records with a genotype and at least one phenotype (records
    without any are removed, :396-404), their rows of the genotype matrix as X (Fortran order, `ftype`), and the individuals EBVs are
    reported for.  Returns ph, rows, X, out_ids, out_rows, out_same; sets Mi.output_rows."""
    geno_index = {g: i for i, g in enumerate(Mi.obsID)}
    keep = np.isfinite(Yall).any(axis=0) & ph[idcol].isin(geno_index).to_numpy()
    ph = ph.loc[keep].reset_index(drop=True)
    if len(ph) == 0:
        raise ValueError("no individual has both phenotypes and genotypes")
    rows = np.array([geno_index[i] for i in ph[idcol]], dtype=np.int64)
    X = np.asfortranarray(np.asarray(Mi.genotypes)[rows, :].astype(ftype))
    out_ids, out_rows, out_same = None, None, True
    if outputEBV:
        out_ids, out_same = resolve_output_ids(model, Mi.obsID, ph[idcol])
        if not out_same:
            out_rows = np.array([geno_index[i] for i in out_ids], dtype=np.int64)
    Mi.output_rows = out_rows if (outputEBV and not out_same) else rows
    return ph, rows, X, out_ids, out_rows, out_same


def open_engine(engine, device, double_precision, X, Mi, out_rows):
    """(the engine with X and, where out_rows names other individuals, their rows loaded; whether it was made here)."""
    own_engine = engine is None
    if own_engine:
        from .engine import HipEngine
        engine = HipEngine(device, precision=64 if double_precision else 32)
    engine.load_dense(X)
    if out_rows is not None:
        engine.load_output_dense(np.asfortranarray(np.asarray(Mi.genotypes)[out_rows, :].astype(X.dtype)))
    return engine, own_engine
