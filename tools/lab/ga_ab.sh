python -m pytest tests/test_fused_gpu.py -m gpu -x -q -k "small_config or ddpm_config or optional" 2>&1 | tail -2
D=$(mktemp -d)
python -m tools.lab.gather_add_bench > $D/new.txt
python -m tools.lab.gather_add_bench --lib point_diffusion_refinement_amd/libpdr_lab.so > $D/prev.txt
paste $D/new.txt $D/prev.txt | awk '{print $1,$2,$3,$4,$5,$6,$7,$8,$9,$10,"|",$(NF-3),$(NF-2)}'
