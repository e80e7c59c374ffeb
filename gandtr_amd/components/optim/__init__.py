"""mirror of mdir/components/optim: the scores a validation without a data loader evaluates (``score``)."""
