"""
Welch spectra and spectral POD of a synthetic cylinder wake with two planted shedding frequencies, on the S^3 grid and on the source
mesh side by side (6 * 10^4 points, 1024 snapshots by default):

    python examples/s3_for_synthetic_spod.py [save_path] [n_snapshots]

The field is exported with ``file_dtype=torch.float32`` and loaded back onto the GPU (``Dataloader.load_snapshot(..., device=True)``);
``welch`` finds the two peaks in the cell-averaged spectrum of the exported field, ``SPOD`` then runs on the exported field (weighted
with the cell areas) and on the float32 source field where it lies, restricted with ``frequencies=`` to the bins around the peaks.
Prints the peaks, the share of the leading SPOD mode at each of them and the sizes of the modes.  Needs an MI355X and the HDF5 sink.
"""
import sys
from os.path import abspath, dirname, join

import numpy as np
import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
from sparsespatialsampling_amd import SPOD, welch                                       # noqa: E402
from sparsespatialsampling_amd.data import Dataloader                                   # noqa: E402
from sparsespatialsampling_amd.export import ExportData                                 # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry, SphereGeometry             # noqa: E402
from sparsespatialsampling_amd.metrics import temporal_std                              # noqa: E402
from sparsespatialsampling_amd.sparse_spatial_sampling import SparseSpatialSampling     # noqa: E402

F_SHED = (3.0, 7.5)             # the two planted frequencies


def wake(xy, n_snapshots, dt):
    """[N, 1, T] float32: two rows of vortices convected downstream of the cylinder at (0.2, 0.2), one per frequency, plus noise"""
    t = pt.arange(n_snapshots, dtype=pt.float64) * dt
    x, y = pt.from_numpy(xy[:, 0] - 0.2), pt.from_numpy(xy[:, 1] - 0.2)
    envelope = pt.exp(-(y / 0.08) ** 2) * pt.sigmoid(40 * x) * pt.exp(-x / 1.5)
    p = pt.zeros((len(xy), n_snapshots), dtype=pt.float64)
    for f, amp, side in zip(F_SHED, (1.0, 0.4), (1.0, -1.0)):
        phase = 2 * np.pi * f * (t[None, :] - x[:, None] / 0.6)
        p += amp * (envelope * pt.tanh(side * y / 0.03 + 0.5))[:, None] * pt.cos(phase)
    p += 1.0 + 1e-2 * pt.randn(p.shape, dtype=pt.float64, generator=pt.Generator().manual_seed(0))
    return p.to(pt.float32).unsqueeze(1)


if __name__ == "__main__":
    save_path = sys.argv[1] if len(sys.argv) > 1 else join("run", "cylinder_synthetic_spod")
    n_snapshots = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    save_name, dt, nperseg = "cylinder_synthetic_spod", 0.01, 256

    rng = np.random.default_rng(1)
    xy = rng.random((60000, 2)) * [2.2, 0.41]
    xy = np.ascontiguousarray(xy[np.hypot(xy[:, 0] - 0.2, xy[:, 1] - 0.2) > 0.05])
    write_times = [str(round(dt * i, 3)) for i in range(n_snapshots)]
    p = wake(xy, n_snapshots, dt)

    geometry = [CubeGeometry("domain", True, [0.0, 0.0], [2.2, 0.41]), SphereGeometry("cylinder", False, [0.2, 0.2], 0.05, refine=True)]
    s_cube = SparseSpatialSampling(pt.from_numpy(xy), temporal_std(p[:, 0, :]).reshape(-1), geometry, save_path, save_name, "cylinder",
                                   uniform_levels=5, n_cells_max=8000, max_delta_level=False)
    s_cube.execute_grid_generation()
    export = ExportData(s_cube, write_times=write_times, file_dtype=pt.float32)
    for t0 in range(0, n_snapshots, 256):
        export.export(pt.from_numpy(xy), p[:, :, t0:t0 + 256], "p", n_snapshots_total=n_snapshots)

    loader = Dataloader(save_path, save_name + ".h5")
    field = loader.load_snapshot("p", device=True)                          # [N_cells, T] float32 on the GPU
    field = field.reshape(field.shape[0], -1)
    area = loader.weights
    print(f"{xy.shape[0]} original points -> {tuple(field.shape)} {field.dtype} on {field.device}")

    # 1. where are the peaks?  PSD per cell, averaged with the cell areas
    freq, psd = welch(field, dt, nperseg=nperseg)
    a = area.to(psd.device, pt.float64).reshape(-1, 1)
    mean_psd = (a * psd).sum(0) / a.sum()
    m = mean_psd.cpu().numpy()
    local = [i for i in range(1, len(m) - 1) if m[i] > m[i - 1] and m[i] >= m[i + 1]]
    peaks = sorted(sorted(local, key=lambda i: -m[i])[:2])
    print("peaks of the cell-averaged PSD at", [round(float(freq[i]), 3) for i in peaks], "planted:", F_SHED)

    # 2. SPOD around the peaks, on the grid and on the source mesh (float32, read where it lies; no cell areas in a synthetic cloud)
    bins = sorted({min(max(i + d, 0), nperseg // 2) for i in peaks for d in (-1, 0, 1)})
    spod_grid = SPOD(field, dt, nperseg, cell_area=area, frequencies=bins)
    spod_orig = SPOD(p[:, 0, :].cuda(), dt, nperseg, frequencies=bins)
    print(f"{spod_grid.n_blocks} segments of {nperseg} snapshots; share of the leading mode:")
    print(f"{'f':>9} {'grid':>9} {'source':>9}")
    for j in range(len(bins)):
        print(f"{float(spod_grid.frequency[j]):>9.3f} {float(spod_grid.energy_fraction()[j, 0]):>9.4f} {float(spod_orig.energy_fraction()[j, 0]):>9.4f}")
    j = bins.index(peaks[0])
    print(f"modes at f = {float(spod_grid.frequency[j]):.3f}: grid {tuple(spod_grid.modes(j, 2).shape)}, source {tuple(spod_orig.modes(j, 2).shape)}")
