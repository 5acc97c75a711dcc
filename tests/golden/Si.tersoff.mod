# tersoff/mod fixture of the tests: silicon, the numbers of Kumagai et al. (2007) as remembered; energies in eV
# El El El  beta alpha h eta beta_ters lambda2 B R D lambda1 A n c1 c2 c3 c4 c5
Si Si Si 1.0 2.3890327 -0.365 1.0 1.0 1.345797 121.00047 3.0 0.3 3.2300135 3281.5905 0.93810551 0.20173476 730418.72 1000000.0 1.0 26.0
