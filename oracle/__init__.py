"""CPU oracle for the TRIBE trimodal-encode hot path.

TEST INFRASTRUCTURE ONLY.  Nothing in the product package
(`algonauts-2025_amd/`) imports this; only `tests/`, `__graft_entry__.smoke()`
and the `cpu_baseline` leg of `bench.py` may.  It is the checker, never the
thing measured or shipped.

Contents
--------
* `tribe_ref`   -- fp32 PyTorch-CPU restatement of the reference arithmetic,
                   function by function, each citing the reference file:line.
* `xt_encoder`  -- restatement of the third-party `x_transformers.Encoder`
                   (absent from /root/reference and from this image) as an
                   `nn.Module` with the library's state_dict key names.

* `attention_ref` -- float64 attention forward / backward, the rounding-error
                   bounds the GPU tests hold the kernels to, and f32 emulations
                   of the kernels' roundings with injectable faults.

* `layout_ref`  -- float64 (and ordered-f32) references of the layout, gather and
                   packing kernels between the GEMMs: im2col, the three rotary
                   modes, the conv module, pools, window means, piece and CSR
                   sums, and a bf16 rounding helper on bit patterns.

* `fp8_ref`     -- the OCP e4m3 decode table and round-to-nearest-even encoder
                   from the format definition (numpy only), the float64 GEMM
                   epilogue in the kernel's operator order, and the j / 8
                   operands whose f32 sums are exact in any order.

* `gemm_ref`    -- the bf16 GEMM's whole descriptor in float64 (the fp8 epilogue
                   plus row_scale, EXP2, MUL_AUX, GELU_BWD, the stored
                   pre-activation, transposed operands, batches, gather1), the
                   integer operands whose f32 sums are exact in any order and
                   under any split of K, and replays of the launcher's stream-K
                   and split-K plans with the case table of the GPU test.

* `autograd_ref` -- float64 statements of the forward and every gradient of the
                   autograd functions (Linear, QKVLinear, FeedForward, the norms,
                   VoxelHead, the losses), their case and branch tables, the
                   bit-exact and per-element bounded criteria, and emulated faults.

* `optim_ref`   -- float64 statements of the Adam / AdamW step (plain and clipped) and
                   of the SWA running average with derived per-element bounds, an
                   overflow rule for non-finite gradients, the case set, and an f32
                   restatement with injectable faults.

Pinning status (see DESIGN.md "Oracle")
---------------------------------------
* Everything that lives in the reference's own files (SubjectLayers,
  aggregate_features, FmriEncoder.forward glue, PearsonLoss, InfoNCE, the
  `_run_step` flatten order, `_aggregate_layers`) is PINNED by golden vectors
  produced by executing those very files (tests/golden/make_golden.py).
* Per-voxel Pearson is PINNED against `scipy.stats.pearsonr`, which is what
  the reference itself calls (algonauts2025/main.py:474-477).
* The encoder internals (`x_transformers`, not vendored, not installed) and
  the `torchmetrics.PearsonCorrCoef` streaming update are PARITY UNPINNED:
  the restatement here defines them.
"""
