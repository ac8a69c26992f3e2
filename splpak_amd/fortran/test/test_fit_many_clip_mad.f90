!> `initialize_many_robust` and `mad_each` of the drop-in module: a batch of a 1-D problem on 16 nodes, an empty problem and the
!! first problem again, xtrap = 1, klo = 2.5, khi = 3, up to 8 passes, regrow = 1.  The problem holds a run of seven raised
!! neighbours.  Checked here: the statuses, the run rejected, both copies with the same bits, fewer points out with regrow than
!! without, maxpass = 0 with the bits of `initialize_many` and unit weights, the median of `mad_each` against a sort, the
!! argument checks and the refusal under set_host.  With two arguments the points come from a file (raw: int64 n, then n x and
!! n y as doubles) and coef, wout, clip and the stats of mad_each on y go to a file (raw doubles) for a caller that compares
!! the bits with another binding.
!!   usage: test_fit_many_clip_mad [points.bin results.bin]
program test_fit_many_clip_mad
    use splpak_module, wp => splpak_wp
    use, intrinsic :: iso_c_binding, only: c_int64_t, c_double
    implicit none
    integer,parameter :: nodes(1) = [16], ncol = 16, nbatch = 3, maxpass = 8
    real(wp),parameter :: xmin(1) = [0.0_wp], xmax(1) = [1.0_wp], klo = 2.5_wp, khi = 3.0_wp
    integer(c_int64_t) :: offsets(nbatch+1), n64
    real(wp),allocatable :: x(:,:), y(:), wout(:), w0(:), srt(:)
    real(wp) :: coef(ncol,nbatch), c0(ncol,nbatch), tmp, med
    real(c_double) :: clip(6,nbatch), clip0(6,nbatch), stats(4,nbatch)
    integer :: ierrors(nbatch), ierror, ip, jp, n, seed, nbad, u, nrun
    character(len=1024) :: fin, fout
    type(splpak_type) :: s, h

    nbad = 0
    seed = 9173
    nrun = 0
    if (command_argument_count() >= 2) then
        call get_command_argument(1, fin)
        call get_command_argument(2, fout)
        open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
        read(u) n64
        n = int(n64)
        allocate(x(1,2*n), y(2*n), wout(2*n), w0(2*n), srt(n))
        read(u) x(1,1:n)
        read(u) y(1:n)
        close(u)
    else
        n = 300
        allocate(x(1,2*n), y(2*n), wout(2*n), w0(2*n), srt(n))
        do ip = 1, n      ! ascending x, so that neighbours in the list are neighbours in x
            x(1,ip) = (real(ip, wp) - 0.5_wp)/real(n, wp)
            y(ip) = sin(3.0_wp*x(1,ip)) + 0.1_wp*(lcg() - 0.5_wp)
        end do
        nrun = 7
        y(141:140+nrun) = y(141:140+nrun) + 1.0_wp
    end if
    x(1,n+1:2*n) = x(1,1:n)
    y(n+1:2*n) = y(1:n)
    offsets = [0_c_int64_t, int(n,c_int64_t), int(n,c_int64_t), int(2*n,c_int64_t)]      ! problem 2 is empty

    ! regrow = 0 first, for the comparison
    call s%initialize_many_robust(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, klo, khi, maxpass, 0, wout, c0, ncol, &
                                  ierrors, ierror, clip=clip0)
    if (ierror /= 105 .or. any(clip0(6,:) /= 0.0_c_double)) nbad = nbad + 1
    coef = -7.0_wp
    wout = -5.0_wp
    call s%initialize_many_robust(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, klo, khi, maxpass, 1, wout, coef, ncol, &
                                  ierrors, ierror, clip=clip)
    if (ierror /= 105) then
        nbad = nbad + 1
        write(*,*) 'initialize_many_robust: ierror ', ierror
    end if
    if (ierrors(1) /= 0 .or. ierrors(2) /= 105 .or. ierrors(3) /= 0) nbad = nbad + 1
    if (any(coef(:,2) /= -7.0_wp) .or. any(clip(:,2) /= 0.0_c_double)) nbad = nbad + 1
    if (any(coef(:,1) /= coef(:,3)) .or. any(wout(1:n) /= wout(n+1:2*n)) .or. any(clip(:,1) /= clip(:,3))) nbad = nbad + 1
    if (any(wout /= 0.0_wp .and. wout /= 1.0_wp)) nbad = nbad + 1
    if (nint(clip(2,1)) /= count(wout(1:n) == 0.0_wp) .or. nint(clip(3,1)) /= count(wout(1:n) /= 0.0_wp)) nbad = nbad + 1
    write(*,'(A,I3,A,I4,A,I4,A,I4,A,ES12.4,A,ES12.4)') ' passes ', nint(clip(1,1)), ', out ', nint(clip(2,1)), ' (regrow 0: ', &
        nint(clip0(2,1)), '), returned ', nint(clip(6,1)), ', s ', clip(4,1), ', med ', clip(5,1)
    if (nint(clip(2,1)) > nint(clip0(2,1))) nbad = nbad + 1
    if (nrun > 0) then      ! the run is rejected, and the points lost beside it without regrow return
        if (any(wout(141:140+nrun) /= 0.0_wp) .or. nint(clip(1,1)) < 2) nbad = nbad + 1
        if (nint(clip(6,1)) < 1 .or. nint(clip(2,1)) >= nint(clip0(2,1))) nbad = nbad + 1
    end if

    ! mad_each on y: the median against a sort of problem 1
    call s%mad_each(nbatch, offsets, y, stats, ierror)
    if (ierror /= 0 .or. nint(stats(1,1)) /= n .or. any(stats(:,2) /= 0.0_c_double) .or. any(stats(:,1) /= stats(:,3))) nbad = nbad + 1
    srt = y(1:n)
    do ip = 2, n
        tmp = srt(ip)
        jp = ip - 1
        do while (jp >= 1)
            if (srt(jp) <= tmp) exit
            srt(jp+1) = srt(jp)
            jp = jp - 1
        end do
        srt(jp+1) = tmp
    end do
    if (mod(n, 2) == 1) then
        med = srt((n + 1)/2)
    else
        med = 0.5_wp*(srt(n/2) + srt(n/2 + 1))
    end if
    if (real(stats(2,1), wp) /= med .or. stats(3,1) <= 0.0_c_double) then
        nbad = nbad + 1
        write(*,*) 'mad_each: median ', stats(2,1), ' sorted ', med
    end if
    if (command_argument_count() >= 2) then
        open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
        write(u) coef
        write(u) wout
        write(u) clip
        write(u) stats
        close(u)
    end if

    ! maxpass = 0: the bits of initialize_many, unit weights out
    call s%initialize_many_robust(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, klo, khi, 0, 1, w0, c0, ncol, ierrors, ierror)
    if (ierror /= 105 .or. any(w0 /= 1.0_wp)) nbad = nbad + 1
    coef = -7.0_wp
    call s%initialize_many(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, coef, ncol, ierrors, ierror)
    if (ierror /= 105 .or. any(coef(:,1) /= c0(:,1)) .or. any(coef(:,3) /= c0(:,3))) nbad = nbad + 1
    ! the argument checks are the library's; under set_host the entries refuse
    call s%initialize_many_robust(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, 0.5_wp, khi, maxpass, 1, wout, coef, ncol, &
                                  ierrors, ierror)
    if (ierror /= -3) nbad = nbad + 1
    call s%initialize_many_robust(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, klo, khi, -1, 1, wout, coef, ncol, ierrors, ierror)
    if (ierror /= -3) nbad = nbad + 1
    call s%mad_each(0, offsets, y, stats, ierror)
    if (ierror /= -3) nbad = nbad + 1
    call h%set_host(.true.)
    call h%initialize_many_robust(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, klo, khi, maxpass, 1, wout, coef, ncol, &
                                  ierrors, ierror)
    if (ierror /= -4) nbad = nbad + 1
    call h%mad_each(nbatch, offsets, y, stats, ierror)
    if (ierror /= -4) nbad = nbad + 1
    if (nbad /= 0) error stop 'FAIL test_fit_many_clip_mad'
    write(*,'(A)') ' PASS test_fit_many_clip_mad'
contains
    real(wp) function lcg()
        seed = mod(seed*1103 + 12345, 65536)
        lcg = real(seed, wp)/65536.0_wp
    end function lcg
end program test_fit_many_clip_mad
