"""Shared helpers for building test inputs (cubed-sphere source tiles, lat-lon targets)."""
import ctypes as C

import numpy as np

import orc

D2R = np.pi / 180
R2D = 180 / np.pi


def ref_gnomonic_corners(ni, centres=False, supergrid=False):
    """C<ni> corners from the REFERENCE generator (create_gnomonic_cubic_grid.c:101 compiled in oracle/_ref),
    with fregrid's read-back (every 2nd supergrid point, degrees * D2R; fregrid_util.c:227-232).
    The generator chats on stderr; that is the reference's behaviour."""
    L = orc.ref()
    nx = 2 * ni
    nxp = nx + 1
    nlon = (C.c_int * 6)(*([nx] * 6))
    nlat = (C.c_int * 6)(*([nx] * 6))
    x = np.zeros(6 * nxp * nxp)
    y = np.zeros(6 * nxp * nxp)
    dx = np.zeros(6 * nx * nxp)
    dy = np.zeros(6 * nxp * nx)
    area = np.zeros(6 * nx * nx)
    adx = np.zeros(6 * nxp * nxp)
    ady = np.zeros(6 * nxp * nxp)
    nest = (C.c_int * 128)()
    dp = C.POINTER(C.c_double)
    f = L.create_gnomonic_cubic_grid
    f.restype = None
    f.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)] + [dp] * 7 + \
                 [C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int] + \
                 [C.POINTER(C.c_int)] * 6 + [C.c_int, C.c_int]
    P = lambda a: a.ctypes.data_as(dp)
    f(b"gnomonic_ed", nlon, nlat, P(x), P(y), P(dx), P(dy), P(area), P(adx), P(ady),
      18.0, 0, 0, 1.0, 0.0, 0.0, 0, nest, nest, nest, nest, nest, nest, 0, 0)
    x = x.reshape(6, nxp, nxp)
    y = y.reshape(6, nxp, nxp)
    if supergrid:
        return x, y                                  # degrees, as make_hgrid writes them
    if centres:                                      # T-cell centres: odd supergrid points (fregrid_util.c:238-243)
        return (np.ascontiguousarray(x[:, ::2, ::2] * D2R), np.ascontiguousarray(y[:, ::2, ::2] * D2R),
                np.ascontiguousarray(x[:, 1::2, 1::2] * D2R), np.ascontiguousarray(y[:, 1::2, 1::2] * D2R))
    return np.ascontiguousarray(x[:, ::2, ::2] * D2R), np.ascontiguousarray(y[:, ::2, ::2] * D2R)


def analytic_field(lon_c, lat_c):
    """10*sin(lon+lat): the field of tests/create_daily_tile_files.c:144, evaluated at cell centres."""
    return 10.0 * np.sin(lon_c + lat_c)


def cell_centres(lonc, latc):
    """Crude cell centres (mean of the 4 corners in 3-D) -- only used to synthesise smooth fields."""
    x = np.cos(latc) * np.cos(lonc)
    y = np.cos(latc) * np.sin(lonc)
    z = np.sin(latc)
    avg = lambda a: 0.25 * (a[:-1, :-1] + a[1:, :-1] + a[:-1, 1:] + a[1:, 1:])
    xm, ym, zm = avg(x), avg(y), avg(z)
    r = np.sqrt(xm * xm + ym * ym + zm * zm)
    lon = np.arctan2(ym, xm)
    lon = np.where(lon < 0, lon + 2 * np.pi, lon)
    return lon, np.arcsin(zm / r)


def c2l_mosaic(fg, name):
    """Small mosaics for the order-2 input preparation at sizes that are no multiple of a block, with nx != ny and with
    unequal tiles: dict(nx, ny, lon, lat [ny+1][nx+1], lont, latt [ny][nx] per tile, contacts).
      'c9', 'c10'  global cubed sphere, 486 / 600 cells, 12 contacts
      'patches'    tile 0 of C14 cut 2 x 2 into patches of nx = 7, ny = 5: 4 contacts, outer edges without one
      'unequal'    low-index corner patches of tiles 0, 1, 2 of C16 with nx = 7, 3, 16 and ny = 5, 11, 2: no contact
      'single'     the last of those alone
      'cuboid'     C12 with tile t subsampled [::sy, ::sx]: contacts between tiles of different sizes, which the reference's
                   setup_boundary does not define (for fg_halo_map's refusal only: never give it to a device)"""
    A = np.ascontiguousarray
    if name in ("c9", "c10"):
        ni = int(name[1:])
        lon, lat, lont, latt = fg.gnomonic_ed_grid(ni)
        nx, ny = [ni] * 6, [ni] * 6
        tiles = [(lon[t], lat[t], lont[t], latt[t]) for t in range(6)]
    elif name == "patches":
        lon, lat, lont, latt = fg.gnomonic_ed_grid(14)
        nx, ny = [7] * 4, [5] * 4
        tiles = []
        for pj in range(2):
            for pi in range(2):
                c = (slice(pj * 5, (pj + 1) * 5 + 1), slice(pi * 7, (pi + 1) * 7 + 1))
                m = (slice(pj * 5, (pj + 1) * 5), slice(pi * 7, (pi + 1) * 7))
                tiles.append((lon[0][c], lat[0][c], lont[0][m], latt[0][m]))
    elif name in ("unequal", "single"):
        lon, lat, lont, latt = fg.gnomonic_ed_grid(16)
        nx, ny = [7, 3, 16], [5, 11, 2]
        tiles = [(lon[t][:ny[t] + 1, :nx[t] + 1], lat[t][:ny[t] + 1, :nx[t] + 1], lont[t][:ny[t], :nx[t]], latt[t][:ny[t], :nx[t]])
                 for t in range(3)]
        if name == "single":
            nx, ny, tiles = nx[2:], ny[2:], tiles[2:]
    elif name == "cuboid":
        lon, lat, lont, latt = fg.gnomonic_ed_grid(12)
        sub = ((1, 2), (3, 2), (3, 1), (2, 1), (2, 3), (1, 3))
        nx, ny = [12 // s[0] for s in sub], [12 // s[1] for s in sub]
        # (the centres are not used by the contact search or the halo map; the subsampled ones only fill the slots)
        tiles = [(lon[t][::sy, ::sx], lat[t][::sy, ::sx], lont[t][::sy, ::sx], latt[t][::sy, ::sx]) for t, (sx, sy) in enumerate(sub)]
    else:
        raise ValueError(name)
    lonc, latc, lonm, latm = ([A(t[k]) for t in tiles] for k in range(4))
    for t in range(len(nx)):
        assert lonc[t].shape == (ny[t] + 1, nx[t] + 1) and lonm[t].shape == (ny[t], nx[t])
    return dict(nx=nx, ny=ny, lon=lonc, lat=latc, lont=lonm, latt=latm, contacts=fg.find_contacts(nx, ny, lonc, latc))
